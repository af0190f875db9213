"""Progressive accumulation on the GPU (kifs_render_accumulate_resume_async, accum::carry_render_kernel), bit for bit: the
bytes of every frame AND the f32 bit patterns of every texel of the plane equal tests/progressive_reference.py -- the
unmodified oracle's linear colour of every sub-frame, carried through a plane pass by pass in np.float32 in the
contract's order -- and, wherever one call can hold the views, the bytes of kifs_render_accumulate_jittered_async /
kifs_render_accumulate_async on the same context.  No tolerance.  Frames are 74 x 45 (ten columns past a tile edge, five
rows past one) unless a case says otherwise; every destination and every plane is pre-filled with a sentinel so that a
missing or a stray store shows.  The scenes are tests/accumulate_cases.py's; tests/test_progressive_reference.py holds the
model to the one-call model on the CPU."""
import ctypes as C

import numpy as np
import pytest

import aa_reference as AA
import accumulate_cases as AC
import accumulate_reference as AR
import jitter_reference as JR
import progressive_reference as PR
from geometry_cases import PIPELINES, Raw

pytestmark = pytest.mark.gpu

W, H = AC.W, AC.H
BAD_ARG, BAD_SIZE = 7, 3
SENT = 0xA5
HOOKS = (9, "render_accumulate_kernel", 0, -1, -1)
SPLITS = (2, 3, 1)  # fewer than four waves busy, a partial round, a lone sub-frame


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


def _cells(cells):
    from kifs_raymarching_amd._lib import KifsSubpixel
    return None if cells is None else (KifsSubpixel * len(cells))(*[KifsSubpixel(i, j) for i, j in cells])


def _hooks(g):
    from kifs_raymarching_amd._lib import lib
    return (lib.kifs_debug_last_kernel(g._ctx), g.debug_last_kernel(), g.debug_last_round_steps(), g.debug_last_group_tiles(),
            g.debug_last_bunny_form())


class Plane:
    """A sentinel-filled plane of `count` frames of `rows` rows: bytes on the device, rows `pitch` bytes apart, frames
    `stride` bytes apart (both may be padded)."""

    def __init__(self, count, rows, w, pad=0, tail=0, fill=SENT):
        import torch
        self.count, self.rows, self.w = count, rows, w
        self.pitch = 16 * w + pad
        self.stride = max(rows, 1) * self.pitch + tail
        self.fill = fill
        self.dev = torch.full((count, self.stride), fill, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

    def host(self):
        """((count, rows, W, 4) float32 texels, every other byte of the allocation)."""
        raw = self.dev.cpu().numpy()
        rows = raw[:, :self.rows * self.pitch].reshape(self.count, self.rows, self.pitch)
        texels = np.ascontiguousarray(rows[:, :, :16 * self.w]).view(np.float32).reshape(self.count, self.rows, self.w, 4)
        rest = np.concatenate([rows[:, :, 16 * self.w:].reshape(self.count, -1), raw[:, self.rows * self.pitch:]], axis=1)
        return texels, rest

    def untouched(self):
        return bool((self.dev.cpu().numpy() == self.fill).all())


def _dest(count, rows, pitch):
    import torch
    dest = torch.full((count, max(rows, 1), pitch), SENT, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return dest


def _resume(g, kifs, cams, samples, grid, cells, plane, prior, options=None, dest=None, y0=0, y1=None, encode=1, pitch=None,
            stream=None, sync=True, sums=None, sums_pitch=None, sums_stride=None, ptrs=None):
    """The raw entry point: one pass over `plane` (a Plane), with a picture into `dest` ((count, rows, pitch) uint8 device
    tensor) or without (dest None).  Returns the status."""
    from kifs_raymarching_amd._lib import OptionsUniform, lib
    h = g.screen_data.height
    y1 = h if y1 is None else y1
    count = len(cams) // samples
    if ptrs is None and dest is not None:
        ptrs = (C.c_void_p * count)(*[dest[i].data_ptr() for i in range(count)])
    pitch = (dest.shape[2] if dest is not None else 0) if pitch is None else pitch
    arr = None if options is None else (OptionsUniform * len(options))(*options)
    st = lib.kifs_render_accumulate_resume_async(
        g._ctx, stream, count, samples, kifs.camera_array(cams), arr, grid, _cells(cells),
        plane.dev.data_ptr() if sums is None else sums, plane.pitch if sums_pitch is None else sums_pitch,
        plane.stride if sums_stride is None else sums_stride, prior, ptrs, pitch, y0, y1, encode)
    if sync:
        assert lib.kifs_synchronize(g._ctx) == 0
    return st


def _one_call(g, kifs, cams, samples, grid, cells, options=None, y0=0, y1=None, encode=1, unjittered=False):
    """kifs_render_accumulate_jittered_async (or the unjittered call) for the same views: (count, rows, W, 4) uint8."""
    from kifs_raymarching_amd._lib import OptionsUniform, lib
    w, h = g.screen_data.width, g.screen_data.height
    y1 = h if y1 is None else y1
    count = len(cams) // samples
    dest = _dest(count, y1 - y0, 4 * w)
    ptrs = (C.c_void_p * count)(*[dest[i].data_ptr() for i in range(count)])
    arr = None if options is None else (OptionsUniform * len(options))(*options)
    if unjittered:
        st = lib.kifs_render_accumulate_async(g._ctx, None, count, samples, kifs.camera_array(cams), arr, ptrs, 4 * w, y0, y1, encode)
    else:
        st = lib.kifs_render_accumulate_jittered_async(g._ctx, None, count, samples, kifs.camera_array(cams), arr, grid, _cells(cells),
                                                       ptrs, 4 * w, y0, y1, encode)
    assert st == 0 and lib.kifs_synchronize(g._ctx) == 0
    return _pixels(dest, w)[0]


def _pixels(dest, w):
    host = dest.cpu().numpy()
    return host[:, :, :4 * w].reshape(host.shape[0], host.shape[1], w, 4), host[:, :, 4 * w:]


def _passes(g, kifs, cams, cells, options, count, samples, splits, grid, plane, dest, y0=0, y1=None, encode=1, picture="last"):
    """The views of one call as passes of `splits` sub-frames per frame over `plane`; a picture from the last pass alone
    (picture="last") or from every pass."""
    cam_passes = PR.pass_views(list(cams), count, samples, splits)
    cell_passes = PR.pass_views(list(cells), count, samples, splits) if cells is not None else [None] * len(splits)
    opt_passes = PR.pass_views(list(options), count, samples, splits) if options is not None else [None] * len(splits)
    prior = 0
    for p, n in enumerate(splits):
        last = p == len(splits) - 1
        st = _resume(g, kifs, cam_passes[p], n, grid, cell_passes[p], plane, prior, options=opt_passes[p],
                     dest=dest if (last or picture == "every") else None, y0=y0, y1=y1, encode=encode)
        assert st == 0 and _hooks(g) == HOOKS, (p, st)
        prior += n
    return prior


_LINEAR = {}  # the oracle's linear sub-frames, computed once per scene and shared by the encodes and tests that use it


def _lin(key, oracle, kifs, screen, cams, options, iters, samples, grid, cells, ext=None):
    if key not in _LINEAR:
        _LINEAR[key] = JR.linear_views(oracle, kifs, screen, cams, options, iters, grid, cells, samples, ext)
        _LINEAR[key].setflags(write=False)
    return _LINEAR[key]


def _same(got, want, what):
    bad = (got != want).any(-1)
    assert got.shape == want.shape and not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:3].tolist(),
                                                        got[bad][:2].tolist(), want[bad][:2].tolist())


def _same_plane(texels, want, total, what):
    """Every f32 bit pattern: the sums, and w == float(total)."""
    assert texels.shape == want.shape, (what, texels.shape, want.shape)
    bad = (texels.view(np.uint32) != want.view(np.uint32)).any(-1)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:3].tolist(), texels[bad][:2].tolist(), want[bad][:2].tolist())
    assert (texels[..., 3] == np.float32(total)).all(), what


def _cells_2x6(kifs, g=3):
    from kifs_raymarching_amd.configs import jitter_cells
    return [c for f in range(2) for c in jitter_cells(g, 6, f)]


@pytest.mark.parametrize("name", PIPELINES)
@pytest.mark.parametrize("encode", [1, 0])
def test_every_pipeline_bit_exact(name, encode, ags, kifs, oracle):
    screen, cam, gui, iters = AC.scene(kifs, name)
    _setup(ags, screen, cam, gui, iters)
    cams, cells = AC.blur_cameras(kifs, cam, 2, 6), _cells_2x6(kifs)
    plane, dest = Plane(2, H, W, pad=48, tail=80), _dest(2, H, 4 * W + 32)
    assert _passes(ags, kifs, cams, cells, None, 2, 6, SPLITS, 3, plane, dest, encode=encode) == 6  # options NULL: the context's
    lin = _lin(("pipeline", name), oracle, kifs, screen, cams, gui, iters, 6, 3, cells)
    want, want_plane, _ = PR.progressive_frames(oracle, kifs, screen, cams, gui, iters, 6, 3, SPLITS, cells, encode, lin=lin)
    frames, padding = _pixels(dest, W)
    _same(frames, want, name)
    _same(frames, _one_call(ags, kifs, cams, 6, 3, cells, encode=encode), (name, "one jittered call"))
    texels, rest = plane.host()
    _same_plane(texels, want_plane, 6, name)
    assert padding.shape[-1] == 32 and (padding == SENT).all() and rest.size == 2 * (48 * H + 80) and (rest == SENT).all()


def test_a_first_pass_is_the_one_call_and_reads_no_plane(ags, kifs, oracle):
    """Identity (a): prior_samples == 0 with a picture, over a plane of NaNs."""
    screen, cam, gui, iters = AC.scene(kifs, "julia_24")
    _setup(ags, screen, cam, gui, iters)
    cams = AC.blur_cameras(kifs, cam, 2, 3)
    for encode in (1, 0):
        # a grid of 1: the pixel centre, the unjittered call's bytes -- with zero cells, and with NULL cells (1 == 1 x 1)
        plain = _one_call(ags, kifs, cams, 3, 0, None, encode=encode, unjittered=True)
        plane, dest = Plane(2, H, W, fill=0xFF), _dest(2, H, 4 * W)
        assert np.isnan(plane.host()[0]).all()
        assert _resume(ags, kifs, cams, 3, 1, [(0, 0)] * 6, plane, 0, dest=dest, encode=encode) == 0 and _hooks(ags) == HOOKS
        _same(_pixels(dest, W)[0], plain, ("zero cells", encode))
        _same(plain, AR.accumulate_frames(oracle, kifs, screen, cams, gui, iters, 3, encode), ("model", encode))
        texels = plane.host()[0]
        assert not np.isnan(texels).any() and (texels[..., 3] == np.float32(3.0)).all()
        batch = _one_call(ags, kifs, cams, 1, 0, None, encode=encode, unjittered=True)  # six frames of one sub-frame
        plane, dest = Plane(6, H, W, fill=0xFF), _dest(6, H, 4 * W)
        assert _resume(ags, kifs, cams, 1, 1, None, plane, 0, dest=dest, encode=encode) == 0
        _same(_pixels(dest, W)[0], batch, ("NULL cells", encode))
        assert (plane.host()[0][..., 3] == np.float32(1.0)).all()
        # a grid of 3: the jittered call's bytes
        cells = [(0, 0), (2, 2), (1, 0), (2, 0), (0, 2), (1, 1)]
        jittered = _one_call(ags, kifs, cams, 3, 3, cells, encode=encode)
        plane, dest = Plane(2, H, W, fill=0xFF), _dest(2, H, 4 * W)
        assert _resume(ags, kifs, cams, 3, 3, cells, plane, 0, dest=dest, encode=encode) == 0
        _same(_pixels(dest, W)[0], jittered, ("g = 3", encode))
        lin = _lin(("first", 0), oracle, kifs, screen, cams, gui, iters, 3, 3, cells)
        want, want_plane, _ = PR.progressive_frames(oracle, kifs, screen, cams, gui, iters, 3, 3, (3,), cells, encode, lin=lin)
        _same(jittered, want, ("g = 3 model", encode))
        _same_plane(plane.host()[0], want_plane, 3, ("g = 3 plane", encode))
        assert (jittered != plain).any()


def test_a_pass_without_a_picture_only_advances_the_plane(ags, kifs, oracle):
    screen, cam, gui, iters = AC.scene(kifs, "julia_24")
    _setup(ags, screen, cam, gui, iters)
    cams, cells = AC.blur_cameras(kifs, cam, 2, 6), _cells_2x6(kifs)
    lin = _lin(("pipeline", "julia_24"), oracle, kifs, screen, cams, gui, iters, 6, 3, cells)
    model = PR.split_views(lin, 2, 6, (4, 2))
    cam_p, cell_p = PR.pass_views(cams, 2, 6, (4, 2)), PR.pass_views(cells, 2, 6, (4, 2))
    plane, dest = Plane(2, H, W), _dest(2, H, 4 * W)
    # (pitch_bytes is ignored without destinations: a value no picture could take)
    assert _resume(ags, kifs, cam_p[0], 4, 3, cell_p[0], plane, 0, dest=None, pitch=3) == 0 and _hooks(ags) == HOOKS
    assert (dest.cpu().numpy() == SENT).all()
    first, total = PR.fold(None, 0, model[0])
    _same_plane(plane.host()[0], first, 4, "after the silent pass")
    assert _resume(ags, kifs, cam_p[1], 2, 3, cell_p[1], plane, 4, dest=dest) == 0
    want, want_plane, _ = PR.progressive_frames(oracle, kifs, screen, cams, gui, iters, 6, 3, (4, 2), cells, lin=lin)
    _same(_pixels(dest, W)[0], want, "the pass with a picture")
    _same_plane(plane.host()[0], want_plane, 6, "the final plane")


def test_150_sub_frames_beyond_the_old_ceiling(ags, kifs, oracle):
    """40 x 13, 2 frames x 150 sub-frames as 64 + 64 + 22 at g = 8: the 64-sample passes take the LDS opt-in of the new
    family, and no single call can hold the frame -- the same NumPy model (accumulate_reference.resolve) says what it is."""
    from kifs_raymarching_amd.configs import jitter_cells, pass_splits
    screen, cam, gui, iters = AC.scene(kifs, "julia_24", 40, 13)
    _setup(ags, screen, cam, gui, iters)
    splits = pass_splits(150)
    assert splits == [64, 64, 22]
    cams = AC.blur_cameras(kifs, cam, 2, 150)
    cells = []
    for f in range(2):
        done = 0
        for n in splits:
            cells.extend(jitter_cells(8, n, f + done))
            done += n
    plane, dest = Plane(2, 13, 40), _dest(2, 13, 4 * 40)
    assert _passes(ags, kifs, cams, cells, None, 2, 150, splits, 8, plane, dest) == 150
    lin = _lin(("views300", 0), oracle, kifs, screen, cams, gui, iters, 150, 8, cells)
    want = np.stack([AA.encode(oracle, m, 1) for m in AR.resolve(lin, 150)])
    _same(_pixels(dest, 40)[0], want, "2 x 150")
    _, want_plane, _ = PR.progressive_frames(oracle, kifs, screen, cams, gui, iters, 150, 8, splits, cells, lin=lin)
    _same_plane(plane.host()[0], want_plane, 150, "2 x 150")
    assert (want[0] != want[1]).any()


def test_band_and_padded_pitches(ags, kifs, oracle):
    """Rows [3, 38) with padded rows on both destinations: the same rows of the whole-frame run, picture and plane."""
    screen, cam, gui, iters = AC.scene(kifs, "julia_24")
    _setup(ags, screen, cam, gui, iters)
    cams, cells = AC.blur_cameras(kifs, cam, 2, 6), _cells_2x6(kifs)
    whole_plane, whole = Plane(2, H, W), _dest(2, H, 4 * W)
    _passes(ags, kifs, cams, cells, None, 2, 6, SPLITS, 3, whole_plane, whole)
    plane, dest = Plane(2, 35, W, pad=32, tail=48), _dest(2, 35, 4 * W + 32)
    _passes(ags, kifs, cams, cells, None, 2, 6, SPLITS, 3, plane, dest, y0=3, y1=38)
    frames, padding = _pixels(dest, W)
    assert frames.shape == (2, 35, W, 4) and (padding == SENT).all()
    _same(frames, _pixels(whole, W)[0][:, 3:38], "band picture")
    texels, rest = plane.host()
    _same_plane(texels, whole_plane.host()[0][:, 3:38], 6, "band plane")
    assert (rest == SENT).all()
    lin = _lin(("pipeline", "julia_24"), oracle, kifs, screen, cams, gui, iters, 6, 3, cells)
    want, want_plane, _ = PR.progressive_frames(oracle, kifs, screen, cams, gui, iters, 6, 3, SPLITS, cells, lin=lin, y0=3, y1=38)
    _same(frames, want, "band model")
    _same_plane(texels, want_plane, 6, "band model plane")
    empty, none = Plane(2, 0, W), _dest(2, 0, 4 * W)  # an empty band: nothing to do, nothing written
    assert _resume(ags, kifs, cams[:4], 2, 3, cells[:4], empty, 0, dest=none, y0=20, y1=20) == 0
    assert empty.untouched() and (none.cpu().numpy() == SENT).all()


@pytest.mark.parametrize("name", ["julia_24", "sphere", "sierpinski"])
def test_per_sub_frame_options(name, ags, kifs, oracle):
    """constant, power and both colours differ per sub-frame, whole tiles miss with differing backgrounds and one sub-frame
    of every frame is turned away; the context holds ANOTHER pipeline's options while the calls are made.  A pixel every
    sub-frame misses holds the fold over the backgrounds, across the passes."""
    screen, cam, gui, iters = AC.scene(kifs, name)
    other = kifs.GuiData(primitive_shape=kifs.PrimitiveShape.Torus) if name != "sphere" else kifs.GuiData(fractal_group=kifs.FractalGroup.JuliaSet)
    _setup(ags, screen, cam, other, iters)
    options, cams = AC.varied(kifs, gui, cam, 2, 6)
    cells = [(1, 0), (0, 1), (1, 1), (0, 0), (1, 0), (0, 1)] * 2
    lin = _lin(("varied", name), oracle, kifs, screen, cams, options, iters, 6, 2, cells)
    for encode in (1, 0):
        plane, dest = Plane(2, H, W), _dest(2, H, 4 * W)
        _passes(ags, kifs, cams, cells, options, 2, 6, SPLITS, 2, plane, dest, encode=encode)
        want, want_plane, _ = PR.progressive_frames(oracle, kifs, screen, cams, options, iters, 6, 2, SPLITS, cells, encode, lin=lin)
        _same(_pixels(dest, W)[0], want, (name, encode))
        texels = plane.host()[0]
        _same_plane(texels, want_plane, 6, (name, encode))
    for f in range(2):  # the fold over the backgrounds, in order, where every sub-frame misses
        bgs = [np.array(list(options[6 * f + s].background_color), dtype=np.float32) for s in range(6)]
        acc = bgs[0].copy()
        for b in bgs[1:]:
            acc = (acc + b).astype(np.float32)
        missed = np.ones((H, W), dtype=bool)
        for s in range(6):
            missed &= (lin[6 * f + s] == bgs[s]).all(-1)
        assert missed.any() and not missed.all()
        assert (texels[f][missed][:, :3].view(np.uint32) == acc.view(np.uint32)).all()
        assert len({tuple(b) for b in bgs}) > 1


def test_heatmap_and_soft_shadows(ags, kifs, oracle):
    screen, cam, gui, iters = AC.scene(kifs, "julia_24")
    heat = kifs.GuiData(**{**gui.__dict__, "is_heatmap": True, "fractal_color": (255, 128, 30)})
    _setup(ags, screen, cam, heat, iters)
    cams, cells = AC.blur_cameras(kifs, cam, 2, 6), _cells_2x6(kifs)
    plane, dest = Plane(2, H, W), _dest(2, H, 4 * W)
    _passes(ags, kifs, cams, cells, None, 2, 6, SPLITS, 3, plane, dest)
    lin = _lin(("heatmap", 0), oracle, kifs, screen, cams, heat, iters, 6, 3, cells)
    want, want_plane, _ = PR.progressive_frames(oracle, kifs, screen, cams, heat, iters, 6, 3, SPLITS, cells, lin=lin)
    _same(_pixels(dest, W)[0], want, "heatmap")
    _same_plane(plane.host()[0], want_plane, 6, "heatmap")
    plain = _lin(("pipeline", "julia_24"), oracle, kifs, screen, cams, gui, iters, 6, 3, cells)
    assert (lin != plain).any()

    screen, cam, gui, iters = AC.scene(kifs, "sierpinski")
    _setup(ags, screen, cam, gui, iters)
    cams = AC.blur_cameras(kifs, cam, 2, 6)
    plane, dest = Plane(2, H, W), _dest(2, H, 4 * W)
    ags.set_extensions(soft_shadow=True, shadow_steps=64, shadow_k=8.0, shadow_t0=0.02, shadow_max_t=10.0)
    try:
        _passes(ags, kifs, cams, cells, None, 2, 6, SPLITS, 3, plane, dest)
    finally:
        ags.set_extensions(soft_shadow=False)
    ext = oracle.Ext(1, 64, 8.0, 0.02, 10.0)
    lin = _lin(("shadow", 0), oracle, kifs, screen, cams, gui, iters, 6, 3, cells, ext=ext)
    want, want_plane, _ = PR.progressive_frames(oracle, kifs, screen, cams, gui, iters, 6, 3, SPLITS, cells, lin=lin)
    _same(_pixels(dest, W)[0], want, "soft shadows")
    _same_plane(plane.host()[0], want_plane, 6, "soft shadows")
    assert (lin != _lin(("pipeline", "sierpinski"), oracle, kifs, screen, cams, gui, iters, 6, 3, cells)).any()


def test_two_passes_of_65_views_go_through_the_view_table(ags, kifs, oracle):
    from kifs_raymarching_amd.configs import jitter_cells
    screen, cam, gui, iters = AC.scene(kifs, "julia_24")
    _setup(ags, screen, cam, kifs.GuiData(), iters)
    options, cams = AC.varied(kifs, gui, cam, 13, 10, seed=1)
    for v in range(len(cams)):  # nearer than `varied` puts them: most of the frame hits
        if v % 10 != 1:
            cams[v] = kifs.CameraData(origin_distance=3.0 + 0.01 * v, phi=0.3 + 0.02 * v, theta=0.2).into_buffer_data()
    cells = [c for f in range(13) for c in jitter_cells(4, 10, f)]
    plane, dest = Plane(13, H, W), _dest(13, H, 4 * W)
    assert _passes(ags, kifs, cams, cells, options, 13, 10, (5, 5), 4, plane, dest) == 10
    lin = _lin(("views130", 0), oracle, kifs, screen, cams, options, iters, 10, 4, cells)
    want, want_plane, _ = PR.progressive_frames(oracle, kifs, screen, cams, options, iters, 10, 4, (5, 5), cells, lin=lin)
    _same(_pixels(dest, W)[0], want, "2 x (13 x 5)")
    _same_plane(plane.host()[0], want_plane, 10, "2 x (13 x 5)")
    assert (want[0] != want[12]).any()


def test_the_library_keeps_no_state(ags, kifs, oracle):
    """Pass 1 from context A, pass 2 from context B on a stream of the caller's ordered after A's, pass 3 from A again:
    the plane and prior_samples are the whole state."""
    import torch
    from kifs_raymarching_amd._lib import lib
    screen, cam, gui, iters = AC.scene(kifs, "julia_24")
    _setup(ags, screen, cam, gui, iters)
    cams, cells = AC.blur_cameras(kifs, cam, 2, 6), _cells_2x6(kifs)
    cam_p, cell_p = PR.pass_views(cams, 2, 6, SPLITS), PR.pass_views(cells, 2, 6, SPLITS)
    plane, dest = Plane(2, H, W), _dest(2, H, 4 * W)
    sa, sb = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    with kifs.GraphicState(0) as other:
        _setup(other, screen, cam, gui, iters)
        assert _resume(ags, kifs, cam_p[0], 2, 3, cell_p[0], plane, 0, stream=sa.cuda_stream, sync=False) == 0
        assert lib.kifs_order_after(other._ctx, sb.cuda_stream, sa.cuda_stream) == 0
        assert _resume(other, kifs, cam_p[1], 3, 3, cell_p[1], plane, 2, stream=sb.cuda_stream, sync=False) == 0
        assert _hooks(other) == HOOKS
        assert lib.kifs_order_after(ags._ctx, sa.cuda_stream, sb.cuda_stream) == 0
        assert _resume(ags, kifs, cam_p[2], 1, 3, cell_p[2], plane, 5, dest=dest, stream=sa.cuda_stream, sync=False) == 0
        sa.synchronize()
        sb.synchronize()
    lin = _lin(("pipeline", "julia_24"), oracle, kifs, screen, cams, gui, iters, 6, 3, cells)
    want, want_plane, _ = PR.progressive_frames(oracle, kifs, screen, cams, gui, iters, 6, 3, SPLITS, cells, lin=lin)
    _same(_pixels(dest, W)[0], want, "A, B, A")
    _same_plane(plane.host()[0], want_plane, 6, "A, B, A")


def test_refusals_write_nothing(ags, kifs):
    screen, cam, gui, iters = AC.scene(kifs, "sierpinski", 40, 24)
    _setup(ags, screen, cam, gui, iters)
    cams = AC.blur_cameras(kifs, cam, 3, 2)
    good = [(0, 0), (2, 2), (1, 0), (2, 0), (0, 2), (1, 1)]

    def refused(want, grid=3, cells=good, samples=2, use=cams, prior=5, picture=True, rows=24, **kw):
        count = len(use) // samples
        plane, dest = Plane(count, rows, 40, pad=16, tail=32), _dest(count, rows, 4 * 40)
        st = _resume(ags, kifs, use, samples, grid, cells, plane, prior, dest=dest if picture else None, **kw)
        assert st == want, (st, grid, cells, kw)
        assert plane.untouched() and (dest.cpu().numpy() == SENT).all(), (grid, cells, kw)
        return plane, dest

    # what the jittered call refuses, with its status
    refused(BAD_ARG, grid=0, cells=[(0, 0)] * 6)
    refused(BAD_ARG, grid=9)
    refused(BAD_ARG, cells=good[:4] + [(3, 0)] + good[5:])
    refused(BAD_ARG, grid=1, cells=[(0, 0)] * 5 + [(1, 0)])
    refused(BAD_ARG, cells=None)                         # NULL cells: 2 samples are not 9
    refused(BAD_ARG, samples=65, use=cams[:1] * 65, cells=[(0, 0)] * 65)  # KIFS_MAX_ACCUMULATE holds per pass
    ags.set_supersampling(2)
    try:
        refused(BAD_ARG)
    finally:
        ags.set_supersampling(1)
    refused(BAD_ARG, encode=2)
    refused(BAD_ARG, y0=5, y1=25)
    refused(BAD_SIZE, pitch=4 * 40 - 4)
    plane, dest = Plane(3, 24, 40), _dest(3, 24, 4 * 40)
    for entry in (0, dest[1].data_ptr() + 2):            # a null and a misaligned ENTRY of a given array
        ptrs = (C.c_void_p * 3)(dest[0].data_ptr(), entry, dest[2].data_ptr())
        assert _resume(ags, kifs, cams, 2, 3, good, plane, 5, dest=dest, ptrs=ptrs) == BAD_ARG
    assert plane.untouched() and (dest.cpu().numpy() == SENT).all()
    # the plane
    base = Plane(3, 24, 40, pad=16, tail=32)
    refused(BAD_ARG, sums=0)
    refused(BAD_ARG, sums=base.dev.data_ptr() + 8)
    refused(BAD_ARG, sums=base.dev.data_ptr() + 4, picture=False)
    refused(BAD_ARG, sums_pitch=16 * 40 - 16)
    refused(BAD_ARG, sums_pitch=16 * 40 + 8)
    refused(BAD_ARG, sums_stride=24 * (16 * 40 + 16) + 8)
    refused(BAD_ARG, sums_stride=24 * (16 * 40 + 16) - 16)   # three frames would overlap
    refused(BAD_ARG, prior=(1 << 24) - 1)                    # + 2 samples: past KIFS_MAX_PROGRESSIVE_SAMPLES
    refused(BAD_ARG, prior=0xFFFFFFFF)
    refused(BAD_ARG, prior=(1 << 24) - 1, picture=False)
    assert base.untouched()
    # and the same arguments unrefused: at the limit itself, with a picture and without (where a bad pitch_bytes is no refusal)
    plane, dest = Plane(3, 24, 40, pad=16, tail=32), _dest(3, 24, 4 * 40)
    assert _resume(ags, kifs, cams, 2, 3, good, plane, (1 << 24) - 2, dest=dest) == 0
    assert not (_pixels(dest, 40)[0] == SENT).all(-1).any()
    texels, rest = plane.host()
    assert (texels[..., 3] == np.float32(1 << 24)).all() and (rest == SENT).all()
    plane = Plane(3, 24, 40)
    assert _resume(ags, kifs, cams, 2, 3, good, plane, 0, dest=None, pitch=4 * 40 - 4) == 0
    assert (plane.host()[0][..., 3] == np.float32(2.0)).all()
    one = Plane(1, 24, 40)  # one frame: the stride is not looked at beyond its alignment
    assert _resume(ags, kifs, cams[:2], 2, 3, good[:2], one, 0, dest=None, sums_stride=0) == 0
    assert (one.host()[0][..., 3] == np.float32(2.0)).all()


def test_the_context_is_left_as_it_was(kifs):
    """A 720p Julia frame has enough tiles for the tile-cost feedback: progressive passes in between neither record costs
    nor move the sort, and the plain frames around them are the same bytes from the same kernel."""
    import torch
    screen, cam, gui, iters = AC.scene(kifs, "julia_24", 1280, 720)
    with kifs.GraphicState(0, screen_data=screen, camera_data=cam, gui_data=gui) as g:
        g.set_iters(*iters)
        frames = [g.render() for _ in range(5)]
        assert all((f == frames[0]).all() for f in frames)
        kernel = g.debug_last_kernel()
        before = g.debug_get_tile_order()
        cams = AC.blur_cameras(kifs, cam, 2, 4)
        acc = kifs.Accumulator(g, count=2)
        first = [cams[0], cams[1], cams[4], cams[5]]
        rest = [cams[2], cams[3], cams[6], cams[7]]
        assert acc.add(first, 2, picture=False, jitter=(2, [(0, 1), (1, 0), (1, 1), (0, 0)])) is None and acc.total == 2
        g.synchronize()
        assert _hooks(g) == HOOKS and (g.debug_get_tile_order() == before).all()
        out = acc.add(rest, 2, jitter=(2, [(1, 1), (0, 0), (0, 1), (1, 0)]))
        g.synchronize()
        assert _hooks(g) == HOOKS and (g.debug_get_tile_order() == before).all() and acc.total == 4
        assert tuple(out.shape) == (2, 720, 1280, 4) and out.dtype == torch.uint8
        # the wrapper's passes are one jittered call's bytes: frame f holds sub-frames (first[2f], first[2f+1], rest[2f], rest[2f+1])
        call_cells = [(0, 1), (1, 0), (1, 1), (0, 0), (1, 1), (0, 0), (0, 1), (1, 0)]
        whole = g.render_accumulate(cams, 4, jitter=(2, call_cells))
        g.synchronize()
        assert (out == whole).all()
        mean = acc.linear_mean()
        assert tuple(mean.shape) == (2, 720, 1280, 3) and bool((acc.sums[..., 3] == 4.0).all())
        acc.reset()
        assert acc.total == 0
        after = g.render()
        assert (after == frames[0]).all() and g.debug_last_kernel() == kernel != "render_accumulate_kernel"
        assert not (out[0] == out[1]).all()


FUZZ = 8


def _fuzz_case(K, seed):
    rng = np.random.default_rng(20261019 + 131 * seed)
    name = PIPELINES[int(rng.integers(0, len(PIPELINES)))]
    w, h = int(rng.integers(9, 49)), int(rng.integers(3, 25))
    g = int(rng.integers(1, K.MAX_JITTER_GRID + 1))
    passes = int(rng.integers(1, 5))
    splits = tuple(int(rng.integers(1, 6)) for _ in range(passes))
    samples = sum(splits)
    count = int(rng.integers(1, 4))
    cells = [(int(rng.integers(0, g)), int(rng.integers(0, g))) for _ in range(count * samples)]
    y0 = int(rng.integers(0, h))
    y1 = int(rng.integers(y0 + 1, h + 1))
    if rng.integers(0, 2):
        y0, y1 = 0, h
    return dict(name=name, w=w, h=h, g=g, splits=splits, samples=samples, count=count, cells=cells, y0=y0, y1=y1,
                encode=int(rng.integers(0, 2)), varied=bool(rng.integers(0, 2)) and name != "unknown_id",
                pad=4 * int(rng.integers(0, 5)), plane_pad=16 * int(rng.integers(0, 4)), every=bool(rng.integers(0, 2)), seed=seed)


@pytest.mark.parametrize("seed", range(FUZZ))
def test_random_progressive_launches(seed, ags, kifs, oracle):
    """Random pipeline, split, grid, cells, band, encode and per-sub-frame options on frames of at most 48 x 24."""
    p = _fuzz_case(kifs, seed)
    screen, cam, gui, iters = AC.scene(kifs, p["name"], p["w"], p["h"])
    _setup(ags, screen, cam, gui, iters)
    count, samples, g = p["count"], p["samples"], p["g"]
    if p["varied"]:
        options, cams = AC.varied(kifs, gui, cam, count, samples, seed=seed)
        for v in range(len(cams)):  # nearer than `varied` puts them, so that rays hit
            if v % samples != 1:
                cams[v] = kifs.CameraData(origin_distance=cam.origin_distance + 0.02 * v, phi=cam.phi + 0.03 * v, theta=cam.theta).into_buffer_data()
    else:
        options, cams = None, AC.blur_cameras(kifs, cam, count, samples)
    rows = p["y1"] - p["y0"]
    plane, dest = Plane(count, rows, p["w"], pad=p["plane_pad"], tail=p["plane_pad"]), _dest(count, rows, 4 * p["w"] + p["pad"])
    total = _passes(ags, kifs, cams, p["cells"], options, count, samples, p["splits"], g, plane, dest, y0=p["y0"], y1=p["y1"],
                    encode=p["encode"], picture="every" if p["every"] else "last")
    assert total == samples
    want, want_plane, _ = PR.progressive_frames(oracle, kifs, screen, cams, options if options is not None else gui, iters, samples, g,
                                                p["splits"], p["cells"], p["encode"], y0=p["y0"], y1=p["y1"])
    frames, padding = _pixels(dest, p["w"])
    assert (padding == SENT).all(), p
    _same(frames, want, p)
    texels, rest = plane.host()
    _same_plane(texels, want_plane, samples, p)
    assert (rest == SENT).all(), p
