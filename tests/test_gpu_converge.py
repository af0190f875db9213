"""Converging accumulation on the GPU (kifs_render_accumulate_converge_async, accum::converge_render_kernel), bit for bit:
every byte of every picture, every f32 bit pattern of both planes and every count equal tests/converge_reference.py --
the unmodified oracle's linear colour of every sub-frame, carried through both planes pass by pass in np.float32 with
the header's rule.  No tolerance.  Frames are 74 x 45 or smaller; every destination, both planes and the words around
the counts are pre-filled with a sentinel so that a missing or a stray store shows, and rows are padded.  What the tests
exist to hold: no active pixel's colour depends on which other pixels are active, and an inactive pixel's two texels keep
their bits.  The cases are tests/converge_cases.py's; tests/test_converge_reference.py shows on the CPU that they mask
pixels, blocks and whole passes."""
import ctypes as C

import numpy as np
import pytest

import accumulate_cases as AC
import converge_cases as CC
import converge_reference as CR
import jitter_reference as JR
import progressive_reference as PR
from geometry_cases import PIPELINES
from test_gpu_progressive import HOOKS, SENT, Plane, _cells, _dest, _hooks, _pixels, _resume, _same, _setup

pytestmark = pytest.mark.gpu

W, H = CC.W, CC.H
BAD_ARG, BAD_SIZE = 7, 3
F = np.float32
GUARD = np.int32(-0x5A5A5A5B)  # 0xA5A5A5A5


@pytest.fixture(scope="module")
def cgs(kifs):
    g = kifs.GraphicState(0)
    yield g
    g.close()


class Sums(Plane):
    def seed(self, texels):
        """The plane's texels from a (count, rows, W, 4) float32 array, bit for bit; everything else stays."""
        import torch
        raw = self.dev.cpu().numpy().copy()
        src = np.ascontiguousarray(texels, dtype=F).view(np.uint8).reshape(self.count, self.rows, 16 * self.w)
        for f in range(self.count):
            raw[f, :self.rows * self.pitch].reshape(self.rows, self.pitch)[:, :16 * self.w] = src[f]
        self.dev.copy_(torch.from_numpy(raw))
        torch.cuda.synchronize()


class Moments:
    """The sentinel-filled plane of one f32 per pixel, laid out as Plane."""

    def __init__(self, count, rows, w, pad=0, tail=0, fill=SENT):
        import torch
        self.count, self.rows, self.w = count, rows, w
        self.pitch = 4 * w + pad
        self.stride = max(rows, 1) * self.pitch + tail
        self.fill = fill
        self.dev = torch.full((count, self.stride), fill, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

    def host(self):
        raw = self.dev.cpu().numpy()
        rows = raw[:, :self.rows * self.pitch].reshape(self.count, self.rows, self.pitch)
        words = np.ascontiguousarray(rows[:, :, :4 * self.w]).view(F).reshape(self.count, self.rows, self.w)
        rest = np.concatenate([rows[:, :, 4 * self.w:].reshape(self.count, -1), raw[:, self.rows * self.pitch:]], axis=1)
        return words, rest

    def seed(self, words):
        import torch
        raw = self.dev.cpu().numpy().copy()
        src = np.ascontiguousarray(words, dtype=F).view(np.uint8).reshape(self.count, self.rows, 4 * self.w)
        for f in range(self.count):
            raw[f, :self.rows * self.pitch].reshape(self.rows, self.pitch)[:, :4 * self.w] = src[f]
        self.dev.copy_(torch.from_numpy(raw))
        torch.cuda.synchronize()

    def untouched(self):
        return bool((self.dev.cpu().numpy() == self.fill).all())


class State:
    """Everything a pass may write: both planes, the counts between two guard words, the destinations."""

    def __init__(self, count, rows, w, pad=0, tail=0, fill=SENT, dest_pad=0):
        import torch
        self.count, self.rows, self.w = count, rows, w
        self.sums = Sums(count, rows, w, pad=16 * pad, tail=16 * tail, fill=fill)
        self.moments = Moments(count, rows, w, pad=4 * pad, tail=4 * tail, fill=fill)
        self.counts = torch.full((count + 2,), int(GUARD), dtype=torch.int32, device="cuda:0")
        self.dest = _dest(count, rows, 4 * w + dest_pad)
        torch.cuda.synchronize()

    def untouched(self):
        return (self.sums.untouched() and self.moments.untouched() and bool((self.counts.cpu().numpy() == GUARD).all())
                and bool((self.dest.cpu().numpy() == SENT).all()))

    def fresh_picture(self):
        self.dest.fill_(SENT)

    def hold(self, want, what, picture=True, counts=True):
        """Everything against one pass of the model (a dict of converge_reference.converged)."""
        texels, rest = self.sums.host()
        assert texels.shape == want["sums"].shape, (what, texels.shape, want["sums"].shape)
        bad = (texels.view(np.uint32) != want["sums"].view(np.uint32)).any(-1)
        assert not bad.any(), (what, "sums", int(bad.sum()), np.argwhere(bad)[:3].tolist(), texels[bad][:2].tolist(),
                               want["sums"][bad][:2].tolist())
        words, mrest = self.moments.host()
        bad = words.view(np.uint32) != want["moments"].view(np.uint32)
        assert not bad.any(), (what, "moments", int(bad.sum()), np.argwhere(bad)[:3].tolist(), words[bad][:2].tolist(),
                               want["moments"][bad][:2].tolist())
        assert (rest == SENT).all() and (mrest == SENT).all(), (what, "plane padding")
        got = self.counts.cpu().numpy()
        assert got[0] == GUARD and got[-1] == GUARD, (what, "count guards")
        if counts:
            assert got[1:-1].tolist() == [int(c) for c in want["counts"]], (what, "counts", got[1:-1].tolist(), want["counts"])
        else:
            assert (got == GUARD).all(), (what, "counts not asked for")
        frames, padding = _pixels(self.dest, self.w)
        assert (padding == SENT).all(), (what, "picture padding")
        if picture:
            _same(frames, want["frames"], (what, "picture"))
        else:
            assert (frames == SENT).all(), (what, "no picture asked for")


def _converge(g, kifs, cams, samples, grid, cells, st, rule, restart, options=None, picture=True, counts=True, y0=0, y1=None,
              encode=1, pitch=None, stream=None, sync=True, sums=None, sums_pitch=None, sums_stride=None, moments=None,
              moments_pitch=None, moments_stride=None, ptrs=None, null_rule=False):
    """The raw entry point: one pass over `st` (a State).  Returns the status."""
    from kifs_raymarching_amd._lib import KifsConvergence, OptionsUniform, lib
    h = g.screen_data.height
    y1 = h if y1 is None else y1
    count = len(cams) // samples
    if ptrs is None and picture:
        ptrs = (C.c_void_p * count)(*[st.dest[i].data_ptr() for i in range(count)])
    pitch = (st.dest.shape[2] if picture else 0) if pitch is None else pitch
    arr = None if options is None else (OptionsUniform * len(options))(*options)
    c_rule = KifsConvergence(rule[0], rule[1])
    status = lib.kifs_render_accumulate_converge_async(
        g._ctx, stream, count, samples, kifs.camera_array(cams), arr, grid, _cells(cells),
        st.sums.dev.data_ptr() if sums is None else sums, st.sums.pitch if sums_pitch is None else sums_pitch,
        st.sums.stride if sums_stride is None else sums_stride,
        st.moments.dev.data_ptr() if moments is None else moments, st.moments.pitch if moments_pitch is None else moments_pitch,
        st.moments.stride if moments_stride is None else moments_stride, int(restart), None if null_rule else C.byref(c_rule),
        st.counts[1:].data_ptr() if counts else None, ptrs, pitch, y0, y1, encode)
    if sync:
        assert lib.kifs_synchronize(g._ctx) == 0
    return status


def _passes(g, kifs, st, cams, cells, options, count, total, splits, grid, rules, want, what, encode=1, y0=0, y1=None,
            restart=True, pictures=True, counts=True):
    """The views of one call as passes of `splits` sub-frames per frame over `st`, pass p under rules[p]; after every
    pass everything is held to want[p]."""
    cam_p = PR.pass_views(list(cams), count, total, splits)
    cell_p = PR.pass_views(list(cells), count, total, splits) if cells is not None else [None] * len(splits)
    opt_p = PR.pass_views(list(options), count, total, splits) if options is not None else [None] * len(splits)
    for p, n in enumerate(splits):
        if pictures:
            st.fresh_picture()
        status = _converge(g, kifs, cam_p[p], n, grid, cell_p[p], st, rules[p], restart and p == 0, options=opt_p[p],
                           picture=pictures, counts=counts, y0=y0, y1=y1, encode=encode)
        assert status == 0 and _hooks(g) == HOOKS, (what, p, status)
        st.hold(want[p], (what, "pass", p), picture=pictures, counts=counts)


_LINEAR = {}  # the oracle's linear sub-frames, computed once per scene and shared, unchanged, by the tests that use it


def _lin(key, oracle, kifs, screen, cams, options, iters, samples, grid, cells, ext=None):
    if key not in _LINEAR:
        _LINEAR[key] = JR.linear_views(oracle, kifs, screen, cams, options, iters, grid, cells, samples, ext)
        _LINEAR[key].setflags(write=False)
    return _LINEAR[key]


def _case(oracle, kifs, name, count=1):
    screen, cam, gui, iters, cams, cells = CC.views(kifs, name, count)
    lin = _lin(("case", name, count), oracle, kifs, screen, cams, gui, iters, CC.SAMPLES, CC.GRID, cells)
    return screen, cam, gui, iters, cams, cells, lin


def _model(oracle, lin, count, rules, encode=1, total=CC.SAMPLES, splits=CC.SPLITS, **kw):
    return CR.converged(oracle, PR.split_views(lin, count, total, splits), rules, encode, **kw)


@pytest.mark.parametrize("name", PIPELINES)
@pytest.mark.parametrize("encode", [1, 0])
def test_every_pipeline_bit_exact(name, encode, cgs, kifs, oracle):
    """Three passes of four at g = 3, min_samples 4, the pipeline's tolerance: pixels, blocks and (julia_24 at 1/8, below)
    whole passes drop out, and every picture, plane bit and count is the model's."""
    screen, cam, gui, iters, cams, cells, lin = _case(oracle, kifs, name)
    _setup(cgs, screen, cam, gui, iters)
    rules = [(CC.tolerance(name), CC.MIN_SAMPLES)] * 3
    want = _model(oracle, lin, 1, rules, encode)
    st = State(1, H, W, pad=3, tail=5, dest_pad=32)
    _passes(cgs, kifs, st, cams, cells, None, 1, CC.SAMPLES, CC.SPLITS, CC.GRID, rules, want, name, encode=encode)
    if CC.TOLERANCE[name] is not None:
        assert 0 < want[2]["counts"][0] < want[0]["counts"][0] < W * H and not want[2]["mask"].all()


def test_two_frames_with_strides(cgs, kifs, oracle):
    screen, cam, gui, iters, cams, cells, lin = _case(oracle, kifs, "sphere", 2)
    _setup(cgs, screen, cam, gui, iters)
    rules = [(CC.tolerance("sphere"), CC.MIN_SAMPLES)] * 3
    want = _model(oracle, lin, 2, rules)
    st = State(2, H, W, pad=1, tail=7, dest_pad=8)
    _passes(cgs, kifs, st, cams, cells, None, 2, CC.SAMPLES, CC.SPLITS, CC.GRID, rules, want, "two frames")
    assert want[2]["counts"][0] != want[2]["counts"][1] and (want[2]["counts"] > 0).all()


def test_identity_a_a_restart_over_nans_is_the_jittered_call(cgs, kifs, oracle):
    from test_gpu_progressive import _one_call
    screen, cam, gui, iters, cams, cells, lin = _case(oracle, kifs, "julia_24")
    _setup(cgs, screen, cam, gui, iters)
    for encode in (1, 0):
        st = State(1, H, W, fill=0xFF)
        assert np.isnan(st.sums.host()[0]).all() and np.isnan(st.moments.host()[0]).all()
        assert _converge(cgs, kifs, cams[:4], 4, CC.GRID, cells[:4], st, (1 / 16, 4), True, encode=encode) == 0
        frames = _pixels(st.dest, W)[0]
        _same(frames, _one_call(cgs, kifs, cams[:4], 4, CC.GRID, cells[:4], encode=encode), ("one jittered call", encode))
        plane = Plane(1, H, W)
        assert _resume(cgs, kifs, cams[:4], 4, CC.GRID, cells[:4], plane, 0, dest=None) == 0
        texels = st.sums.host()[0]
        assert (texels.view(np.uint32) == plane.host()[0].view(np.uint32)).all() and not np.isnan(st.moments.host()[0]).any()
        want = _model(oracle, lin[:4], 1, [(1 / 16, 4)], encode, total=4, splits=(4,))
        assert (texels.view(np.uint32) == want[0]["sums"].view(np.uint32)).all()
        assert (st.moments.host()[0].view(np.uint32) == want[0]["moments"].view(np.uint32)).all()
        assert st.counts.cpu().numpy()[1] == want[0]["counts"][0]


def test_identity_b_nothing_settles_below_min_samples(cgs, kifs, oracle):
    """min_samples above every count reached: the resume call's plane and pictures, pass by pass, on the same context."""
    screen, cam, gui, iters, cams, cells, lin = _case(oracle, kifs, "genjulia")
    _setup(cgs, screen, cam, gui, iters)
    rules = [(np.inf, 13)] * 3
    want = _model(oracle, lin, 1, rules)
    st = State(1, H, W)
    cam_p, cell_p = PR.pass_views(cams, 1, 12, CC.SPLITS), PR.pass_views(cells, 1, 12, CC.SPLITS)
    plane, prior = Plane(1, H, W), 0
    for p in range(3):
        st.fresh_picture()
        assert _converge(cgs, kifs, cam_p[p], 4, CC.GRID, cell_p[p], st, rules[p], p == 0) == 0
        st.hold(want[p], ("b", p))
        dest = _dest(1, H, 4 * W)
        assert _resume(cgs, kifs, cam_p[p], 4, CC.GRID, cell_p[p], plane, prior, dest=dest) == 0
        prior += 4
        _same(_pixels(st.dest, W)[0], _pixels(dest, W)[0], ("resume picture", p))
        assert (st.sums.host()[0].view(np.uint32) == plane.host()[0].view(np.uint32)).all()
        assert want[p]["counts"].tolist() == [W * H]


def test_identity_c_and_a_pass_with_nothing_active(cgs, kifs, oracle):
    """Tolerance +inf, min_samples 8: everything stops after pass 2.  Pass 3 marches nothing, with a picture and without:
    the planes keep their bits, the picture is still complete, the counts are zero."""
    screen, cam, gui, iters, cams, cells, lin = _case(oracle, kifs, "julia_24")
    _setup(cgs, screen, cam, gui, iters)
    rules = [(np.inf, 8)] * 3
    want = _model(oracle, lin, 1, rules)
    assert [int(w["counts"][0]) for w in want] == [W * H, 0, 0] and not want[2]["mask"].any()
    for encode in (1, 0):
        st = State(1, H, W, pad=2, tail=1, dest_pad=16)
        want = _model(oracle, lin, 1, rules, encode)
        _passes(cgs, kifs, st, cams, cells, None, 1, 12, CC.SPLITS, CC.GRID, rules, want, ("c", encode), encode=encode)
        st.fresh_picture()
        st.counts[1] = 77
        assert _converge(cgs, kifs, cams[8:], 4, CC.GRID, cells[8:], st, rules[2], False, picture=False, encode=encode) == 0
        st.hold(want[2], ("c, no picture", encode), picture=False)


def test_inactive_pixels_keep_their_bits_and_frozen_pixels_freeze(cgs, kifs, oracle):
    """The planes seeded from the model after pass 1; then every third pixel is FROZEN at n = 2^24 with sentinel bit
    patterns for its sums and moment, and every seventh stands at 2^24 - 2: a pass of 4 must leave both kinds alone, a
    pass of 2 must take the second kind to 2^24 exactly, where it stays."""
    screen, cam, gui, iters, cams, cells, lin = _case(oracle, kifs, "julia_24")
    _setup(cgs, screen, cam, gui, iters)
    rule = (1 / 16, 4)
    first = _model(oracle, lin, 1, [rule] * 3)[0]
    sums, moments = first["sums"].copy(), first["moments"].copy()
    idx = np.arange(H * W).reshape(1, H, W)
    frozen, near = idx % 3 == 0, (idx % 7 == 0) & (idx % 3 != 0)
    sums.view(np.uint32)[frozen] = 0xA5A5A5A5
    sums[..., 3][frozen] = F(16777216.0)
    moments.view(np.uint32)[frozen] = 0xA5A5A5A5
    sums[..., 3][near] = F(16777214.0)
    moments[near] = F(1.0e30)  # far from settled: only the limit can stop them
    passes = PR.split_views(lin, 1, 12, CC.SPLITS)
    for samples, at in ((4, passes[1]), (2, passes[1][:, :2])):
        want = CR.converged(oracle, [at, at], [rule, rule], sums=sums, moments=moments, restart=False)
        st = State(1, H, W, pad=1)
        st.sums.seed(sums)
        st.moments.seed(moments)
        for p in range(2):
            st.fresh_picture()
            assert _converge(cgs, kifs, cams[4:4 + samples], samples, CC.GRID, cells[4:4 + samples], st, rule, False) == 0
            st.hold(want[p], ("frozen", samples, p))
        texels = st.sums.host()[0]
        assert (texels.view(np.uint32)[frozen][:, :3] == 0xA5A5A5A5).all() and (texels[..., 3][frozen] == F(16777216.0)).all()
        assert (st.moments.host()[0].view(np.uint32)[frozen] == 0xA5A5A5A5).all()
        marched = want[0]["mask"]
        assert not marched[frozen].any() and marched.any()
        if samples == 4:
            assert not marched[near].any() and (texels[..., 3][near] == F(16777214.0)).all()
        else:
            assert marched[near].any() and (texels[..., 3][near & marched] == F(16777216.0)).all() and not want[1]["mask"][near].any()


def test_64_sub_frames_and_150_beyond_the_lds_opt_in(cgs, kifs, oracle):
    """40 x 13, 2 frames x 150 sub-frames as 64 + 64 + 22 at g = 8: the 64-sample passes take the LDS opt-in of the new
    family."""
    from kifs_raymarching_amd.configs import jitter_cells, pass_splits
    screen, cam, gui, iters = AC.scene(kifs, "julia_24", 40, 13)
    _setup(cgs, screen, cam, gui, iters)
    splits = pass_splits(150)
    cams = AC.blur_cameras(kifs, cam, 2, 150)
    cells = []
    for f in range(2):
        done = 0
        for n in splits:
            cells.extend(jitter_cells(8, n, f + done))
            done += n
    lin = _lin(("views300", 0), oracle, kifs, screen, cams, gui, iters, 150, 8, cells)
    rules = [(1 / 64, 64)] * 3
    want = _model(oracle, lin, 2, rules, total=150, splits=splits)
    assert 0 < want[0]["counts"].sum() < 2 * 40 * 13 and 0 < want[1]["mask"].sum() < 2 * 40 * 13
    st = State(2, 13, 40, pad=1, tail=2)
    _passes(cgs, kifs, st, cams, cells, None, 2, 150, splits, 8, rules, want, "2 x 150")
    one = State(2, 13, 40)  # and one pass of 64 on its own
    assert _converge(cgs, kifs, PR.pass_views(cams, 2, 150, splits)[0], 64, 8, PR.pass_views(cells, 2, 150, splits)[0], one,
                     rules[0], True) == 0
    one.hold(want[0], "1 x 64")


def test_band_and_padded_pitches(cgs, kifs, oracle):
    """Rows [3, 38) with padded rows on all three destinations: block rows start at the band's first row."""
    screen, cam, gui, iters, cams, cells, lin = _case(oracle, kifs, "julia_24")
    _setup(cgs, screen, cam, gui, iters)
    rules = [(1 / 16, 4)] * 3
    want = _model(oracle, lin, 1, rules, y0=3, y1=38)
    st = State(1, 35, W, pad=2, tail=3, dest_pad=32)
    _passes(cgs, kifs, st, cams, cells, None, 1, 12, CC.SPLITS, CC.GRID, rules, want, "band", y0=3, y1=38)
    whole = _model(oracle, lin, 1, rules)
    assert (want[2]["sums"].view(np.uint32) == whole[2]["sums"][:, 3:38].view(np.uint32)).all()
    empty = State(1, 0, W)  # an empty band: nothing enqueued, the counts untouched
    assert _converge(cgs, kifs, cams[:4], 4, CC.GRID, cells[:4], empty, rules[0], True, y0=20, y1=20) == 0
    assert empty.untouched()


@pytest.mark.parametrize("name", ["julia_24", "sphere", "sierpinski"])
def test_per_sub_frame_options(name, cgs, kifs, oracle):
    """constant, power and both colours differ per sub-frame and one sub-frame of every frame is turned away; the context
    holds ANOTHER pipeline's options while the calls are made."""
    screen, cam, gui, iters = AC.scene(kifs, name)
    other = kifs.GuiData(primitive_shape=kifs.PrimitiveShape.Torus) if name != "sphere" else kifs.GuiData(fractal_group=kifs.FractalGroup.JuliaSet)
    _setup(cgs, screen, cam, other, iters)
    options, cams = AC.varied(kifs, gui, cam, 2, 6)
    cells = [(1, 0), (0, 1), (1, 1), (0, 0), (1, 0), (0, 1)] * 2
    lin = _lin(("varied", name), oracle, kifs, screen, cams, options, iters, 6, 2, cells)
    rules = [(1 / 16, 2)] * 3
    want = _model(oracle, lin, 2, rules, total=6, splits=(2, 2, 2))
    assert 0 < want[1]["mask"].sum() < 2 * W * H
    st = State(2, H, W)
    _passes(cgs, kifs, st, cams, cells, options, 2, 6, (2, 2, 2), 2, rules, want, name)


def test_heatmap_and_soft_shadows(cgs, kifs, oracle):
    screen, cam, gui, iters, cams, cells, _ = _case(oracle, kifs, "julia_24")
    heat = kifs.GuiData(**{**gui.__dict__, "is_heatmap": True, "fractal_color": (255, 128, 30)})
    _setup(cgs, screen, cam, heat, iters)
    rules = [(1 / 16, 4)] * 3
    lin = _lin(("heatmap", 0), oracle, kifs, screen, cams, heat, iters, 12, CC.GRID, cells)
    want = _model(oracle, lin, 1, rules)
    assert 0 < want[1]["mask"].sum() < W * H
    _passes(cgs, kifs, State(1, H, W), cams, cells, None, 1, 12, CC.SPLITS, CC.GRID, rules, want, "heatmap")

    screen, cam, gui, iters, cams, cells, plain = _case(oracle, kifs, "sierpinski")
    _setup(cgs, screen, cam, gui, iters)
    cgs.set_extensions(soft_shadow=True, shadow_steps=64, shadow_k=8.0, shadow_t0=0.02, shadow_max_t=10.0)
    try:
        ext = oracle.Ext(1, 64, 8.0, 0.02, 10.0)
        lin = _lin(("shadow", 0), oracle, kifs, screen, cams, gui, iters, 12, CC.GRID, cells, ext=ext)
        want = _model(oracle, lin, 1, rules)
        assert 0 < want[1]["mask"].sum() < W * H and (lin != plain).any()
        _passes(cgs, kifs, State(1, H, W), cams, cells, None, 1, 12, CC.SPLITS, CC.GRID, rules, want, "soft shadows")
    finally:
        cgs.set_extensions(soft_shadow=False)


def test_the_tolerance_tightened_between_passes(cgs, kifs, oracle):
    screen, cam, gui, iters, cams, cells, lin = _case(oracle, kifs, "julia_24")
    _setup(cgs, screen, cam, gui, iters)
    rules = [(1 / 8, 4), (1 / 64, 4), (1 / 64, 4)]
    want = _model(oracle, lin, 1, rules)
    loose = _model(oracle, lin, 1, [(1 / 8, 4)] * 3)
    assert want[1]["mask"].sum() > loose[1]["mask"].sum()  # pixels settled at 1/8 are marched again at 1/64
    _passes(cgs, kifs, State(1, H, W), cams, cells, None, 1, 12, CC.SPLITS, CC.GRID, rules, want, "tightened")


def test_two_contexts_and_two_streams_on_one_pair_of_planes(cgs, kifs, oracle):
    """Identity (d): pass 1 from context A, pass 2 from context B on another stream ordered after A's, pass 3 from A."""
    import torch
    from kifs_raymarching_amd._lib import lib
    screen, cam, gui, iters, cams, cells, lin = _case(oracle, kifs, "julia_24")
    _setup(cgs, screen, cam, gui, iters)
    rules = [(1 / 16, 4)] * 3
    want = _model(oracle, lin, 1, rules)
    cam_p, cell_p = PR.pass_views(cams, 1, 12, CC.SPLITS), PR.pass_views(cells, 1, 12, CC.SPLITS)
    st = State(1, H, W)
    sa, sb = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    with kifs.GraphicState(0) as other:
        _setup(other, screen, cam, gui, iters)
        assert _converge(cgs, kifs, cam_p[0], 4, CC.GRID, cell_p[0], st, rules[0], True, stream=sa.cuda_stream, sync=False, picture=False) == 0
        assert lib.kifs_order_after(other._ctx, sb.cuda_stream, sa.cuda_stream) == 0
        assert _converge(other, kifs, cam_p[1], 4, CC.GRID, cell_p[1], st, rules[1], False, stream=sb.cuda_stream, sync=False, picture=False) == 0
        assert _hooks(other) == HOOKS
        assert lib.kifs_order_after(cgs._ctx, sa.cuda_stream, sb.cuda_stream) == 0
        assert _converge(cgs, kifs, cam_p[2], 4, CC.GRID, cell_p[2], st, rules[2], False, stream=sa.cuda_stream, sync=False) == 0
        sa.synchronize()
        sb.synchronize()
    st.hold(want[2], "A, B, A")


def test_without_counts(cgs, kifs, oracle):
    screen, cam, gui, iters, cams, cells, lin = _case(oracle, kifs, "torus")
    _setup(cgs, screen, cam, gui, iters)
    rules = [(CC.tolerance("torus"), 4)] * 3
    want = _model(oracle, lin, 1, rules)
    _passes(cgs, kifs, State(1, H, W), cams, cells, None, 1, 12, CC.SPLITS, CC.GRID, rules, want, "NULL counts", counts=False)


def test_refusals_write_nothing(cgs, kifs):
    screen, cam, gui, iters = AC.scene(kifs, "sierpinski", 40, 24)
    _setup(cgs, screen, cam, gui, iters)
    cams = AC.blur_cameras(kifs, cam, 3, 2)
    good = [(0, 0), (2, 2), (1, 0), (2, 0), (0, 2), (1, 1)]

    def refused(want, grid=3, cells=good, samples=2, use=cams, rule=(1 / 16, 4), restart=False, rows=24, **kw):
        st = State(len(use) // samples, rows, 40, pad=1, tail=2)
        status = _converge(cgs, kifs, use, samples, grid, cells, st, rule, restart, **kw)
        assert status == want, (status, grid, cells, rule, kw)
        assert st.untouched(), (grid, cells, rule, kw)

    # what the resume call refuses, with its status
    refused(BAD_ARG, grid=0, cells=[(0, 0)] * 6)
    refused(BAD_ARG, grid=9)
    refused(BAD_ARG, cells=good[:4] + [(3, 0)] + good[5:])
    refused(BAD_ARG, cells=None)                         # NULL cells: 2 samples are not 9
    refused(BAD_ARG, samples=65, use=cams[:1] * 65, cells=[(0, 0)] * 65)
    cgs.set_supersampling(2)
    try:
        refused(BAD_ARG)
    finally:
        cgs.set_supersampling(1)
    refused(BAD_ARG, encode=2)
    refused(BAD_ARG, y0=5, y1=25)
    refused(BAD_SIZE, pitch=4 * 40 - 4)
    base = State(3, 24, 40, pad=1, tail=2)
    ptrs = (C.c_void_p * 3)(base.dest[0].data_ptr(), 0, base.dest[2].data_ptr())
    refused(BAD_ARG, ptrs=ptrs)
    refused(BAD_ARG, sums=0)
    refused(BAD_ARG, sums=base.sums.dev.data_ptr() + 8)
    refused(BAD_ARG, sums_pitch=16 * 40 - 16)
    refused(BAD_ARG, sums_pitch=16 * 40 + 8)
    refused(BAD_ARG, sums_stride=24 * (16 * 40 + 16) - 16)   # three frames would overlap
    # the moments plane, the rule
    refused(BAD_ARG, moments=0)
    refused(BAD_ARG, moments=base.moments.dev.data_ptr() + 2)
    refused(BAD_ARG, moments=base.moments.dev.data_ptr() + 1, picture=False, restart=True)
    refused(BAD_ARG, moments_pitch=4 * 40 - 4)
    refused(BAD_ARG, moments_pitch=4 * 40 + 2)
    refused(BAD_ARG, moments_stride=24 * (4 * 40 + 4) + 2)
    refused(BAD_ARG, moments_stride=24 * (4 * 40 + 4) - 4)   # three frames would overlap
    refused(BAD_ARG, null_rule=True)
    refused(BAD_ARG, rule=(float("nan"), 4))
    refused(BAD_ARG, rule=(-1 / 16, 4))
    refused(BAD_ARG, rule=(1 / 16, 1))
    refused(BAD_ARG, rule=(1 / 16, 0))
    refused(BAD_ARG, rule=(1 / 16, (1 << 24) + 1), counts=False)
    assert base.untouched()
    # and the same arguments unrefused, at the limits themselves
    for rule in ((float("inf"), 1 << 24), (0.0, 3)):
        st = State(3, 24, 40, pad=1, tail=2)
        assert _converge(cgs, kifs, cams, 2, 3, good, st, rule, True) == 0
        assert not (_pixels(st.dest, 40)[0] == SENT).all(-1).any() and (st.sums.host()[0][..., 3] == 2.0).all()
        assert st.counts.cpu().numpy()[1:-1].tolist() == [40 * 24] * 3
    one = State(1, 24, 40)  # one frame: the strides are not looked at beyond their alignment
    assert _converge(cgs, kifs, cams[:2], 2, 3, good[:2], one, (1 / 16, 2), True, picture=False, pitch=3, sums_stride=0, moments_stride=0) == 0
    assert (one.sums.host()[0][..., 3] == 2.0).all()


def test_the_context_is_left_as_it_was(kifs, oracle):
    """The plain path's order, kernel and bytes around converging passes."""
    screen, cam, gui, iters = AC.scene(kifs, "julia_24", 320, 184)
    with kifs.GraphicState(0, screen_data=screen, camera_data=cam, gui_data=gui) as g:
        g.set_iters(*iters)
        frames = [g.render() for _ in range(3)]
        assert all((f == frames[0]).all() for f in frames)
        kernel, before = g.debug_last_kernel(), g.debug_get_tile_order()
        acc = kifs.ConvergingAccumulator(g, count=1, tolerance=1 / 16, min_samples=4)
        cams = AC.blur_cameras(kifs, cam, 1, 8)
        assert acc.add(cams[:4], 4, picture=False, jitter=(2, [(0, 1), (1, 0), (1, 1), (0, 0)])) is None
        first = acc.active()
        out = acc.add(cams[4:], 4, jitter=(2, [(1, 1), (0, 0), (0, 1), (1, 0)]))
        left = acc.active()
        assert _hooks(g) == HOOKS and (g.debug_get_tile_order() == before).all() and acc.total == 8
        assert 0 < left[0] <= first[0] < 320 * 184 and tuple(out.shape) == (1, 184, 320, 4)
        n = acc.samples_per_pixel().cpu().numpy()
        assert set(np.unique(n).tolist()) == {4.0, 8.0} and int((n == 8.0).sum()) == first[0]
        after = g.render()
        assert (after == frames[0]).all() and g.debug_last_kernel() == kernel != "render_accumulate_kernel"


FUZZ = 8


def _fuzz_case(K, seed):
    rng = np.random.default_rng(20261020 + 977 * seed)
    name = PIPELINES[int(rng.integers(0, len(PIPELINES)))]
    w, h = int(rng.integers(9, 49)), int(rng.integers(3, 25))
    g = int(rng.integers(1, K.MAX_JITTER_GRID + 1))
    count, samples = int(rng.integers(1, 4)), int(rng.integers(1, 7))
    cells = [(int(rng.integers(0, g)), int(rng.integers(0, g))) for _ in range(count * samples)]
    y0 = int(rng.integers(0, h))
    y1 = int(rng.integers(y0 + 1, h + 1))
    if rng.integers(0, 2):
        y0, y1 = 0, h
    return dict(name=name, w=w, h=h, g=g, samples=samples, count=count, cells=cells, y0=y0, y1=y1, encode=int(rng.integers(0, 2)),
                pad=int(rng.integers(0, 4)), picture=bool(rng.integers(0, 4)), counts=bool(rng.integers(0, 4)),
                density=float(rng.choice([0.02, 0.3, 0.7, 1.0])), seed=seed), rng


def _random_state(rng, count, rows, w, density):
    """(the mask, the sums plane, the moments plane) of a random state: a pixel off the mask is frozen (n = 2^24, arbitrary
    finite bit patterns in its sums) or settled (n identical grey samples), whole 8 x 8 blocks among them; a pixel on it
    holds random sums far from settled."""
    shape = (count, rows, w)
    on = rng.random(shape) < density
    for _ in range(3):  # whole blocks off
        by, bx = 8 * int(rng.integers(0, (rows + 7) // 8)), 8 * int(rng.integers(0, (w + 7) // 8))
        on[int(rng.integers(0, count)), by:by + 8, bx:bx + 8] = False
    n = rng.integers(2, 40, shape).astype(F)
    grey = rng.random(shape).astype(F)
    sums = np.empty(shape + (4,), dtype=F)
    sums[..., :3] = rng.random(shape + (3,)).astype(F) * n[..., None]
    sums[..., 3] = n
    moments = (F(4.0) * n * n).astype(F)                      # far from settled: d = n q - L^2 >= 3 n^3 > b
    settled = ~on & (rng.random(shape) < 0.5)                 # n identical grey samples: d about 0 <= b
    sums[..., :3][settled] = (grey * n)[settled][:, None]
    y = CR.luminance(np.stack([grey] * 3, -1))
    moments[settled] = (n * y * y).astype(F)[settled]
    frozen = ~on & ~settled
    sums.view(np.uint32)[..., :3][frozen] = rng.integers(0, 1 << 32, (int(frozen.sum()), 3), dtype=np.uint64).astype(np.uint32) & 0x7F7FFFFF
    sums[..., 3][frozen] = F(16777216.0)
    return on, sums, moments


@pytest.mark.parametrize("seed", range(FUZZ))
def test_random_masks(seed, cgs, kifs, oracle):
    """Random pipeline, grid, cells, band and encode on frames of at most 48 x 24 over planes seeded with RANDOM masks: a
    pixel is made inactive by freezing it (n = 2^24, arbitrary bit patterns in its sums and moment) or by a settled state
    (identical samples), whole 8 x 8 blocks among them; the active ones hold random sums far from settled."""
    p, rng = _fuzz_case(kifs, seed)
    screen, cam, gui, iters = AC.scene(kifs, p["name"], p["w"], p["h"])
    _setup(cgs, screen, cam, gui, iters)
    count, samples, rows, w = p["count"], p["samples"], p["y1"] - p["y0"], p["w"]
    cams = AC.blur_cameras(kifs, cam, count, samples)
    lin = JR.linear_views(oracle, kifs, screen, cams, gui, iters, p["g"], p["cells"], samples)
    on, sums, moments = _random_state(rng, count, rows, w, p["density"])
    rule = (1 / 16, 2)
    assert (CR.active(sums, moments, rule, samples) == on).all(), p
    want = CR.converged(oracle, [lin.reshape(count, samples, *lin.shape[1:])], [rule], p["encode"], p["y0"], p["y1"], sums=sums,
                        moments=moments, restart=False)[0]
    st = State(count, rows, w, pad=p["pad"], tail=p["pad"], dest_pad=4 * p["pad"])
    st.sums.seed(sums)
    st.moments.seed(moments)
    assert _converge(cgs, kifs, cams, samples, p["g"], p["cells"], st, rule, False, picture=p["picture"], counts=p["counts"],
                     y0=p["y0"], y1=p["y1"], encode=p["encode"]) == 0
    st.hold(want, p, picture=p["picture"], counts=p["counts"])
