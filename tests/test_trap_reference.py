"""tests/trap_reference.c IS the contract of kifs_render_trapped_async on the oracle.  With scale = bias = 0 its frame is
tests/lighting_reference.c's bit for bit, for the reference's light and the test light A, with and without a term, and
with the reference's light it is kor_render_ext's bytes; u of the sphere with a point trap at the origin and no orbit is
sqrtf of the f32 sum of squares of the position; and the two test traps do colour the GPU tests' frames: among their hit
pixels there are many distinct values of t, hits in both segments of the gradient and, for the Julia trap, saturated
pixels at both ends.  That is what makes the GPU comparison of tests/test_gpu_trap.py mean something.  CPU only."""
import numpy as np
import pytest

import lighting_reference as LR
import occlusion_reference as OR
import trap_reference as TR
from geometry_cases import PIPELINES, cases
from helpers import oracle_uniforms
from test_occlusion_reference import _fma32

GW, GH = 102, 45       # the frames of the GPU tests
f32 = np.float32


def _ext(oracle, on):
    return oracle.Ext(1, 64, 8.0, 0.02, 10.0) if on else None


@pytest.mark.parametrize("ao", [None, OR.DEFAULT], ids=["bare", "term"])
@pytest.mark.parametrize("spec_name", ["REFERENCE", "A"])
@pytest.mark.parametrize("name", PIPELINES)
def test_a_flat_gradient_is_the_lighting_models_frame(name, spec_name, ao, kifs, oracle):
    screen, cam, gui, iters = cases(kifs, GW, GH)[name]
    s, c, o = oracle_uniforms(oracle, kifs, (screen, cam, gui))
    it = oracle.iters(*iters)
    spec = getattr(LR, spec_name)
    flat = dict(TR.for_scene(name), scale=0.0, bias=0.0)
    want = LR.march(oracle, s, c, o, it, spec, ao, None)
    got = TR.march(oracle, s, c, o, it, flat, spec, ao, None)
    assert (got.hit == want.hit).all() and TR.same_bits(got.pos, want.pos).all()
    assert TR.same_bits(got.rgb, want.rgb).all(), (name, spec_name, ao)
    assert (got.t[got.hit] == 0).all()
    if spec_name == "REFERENCE" and ao is None:
        null = TR.march(oracle, s, c, o, it, flat, None, None, None)  # a NULL light is the reference's
        assert TR.same_bits(null.rgb, want.rgb).all()
        for encode in (1, 0):
            assert (TR.encode(oracle, got.rgb, encode) == oracle.render(s, c, o, it, encode=encode)).all(), (name, encode)


@pytest.mark.parametrize("name", ["julia_24", "sierpinski"])
def test_a_flat_gradient_with_shadows_and_same_stops(name, kifs, oracle):
    """Identity (a) with the soft-shadow extension, and identity (b): mid = far = fractal_color with any range."""
    screen, cam, gui, iters = cases(kifs, GW, GH)[name]
    s, c, o = oracle_uniforms(oracle, kifs, (screen, cam, gui))
    it = oracle.iters(*iters)
    want = LR.march(oracle, s, c, o, it, LR.A, OR.DEFAULT, _ext(oracle, True))
    flat = dict(TR.for_scene(name), scale=0.0, bias=0.0)
    assert TR.same_bits(TR.march(oracle, s, c, o, it, flat, LR.A, OR.DEFAULT, _ext(oracle, True)).rgb, want.rgb).all()
    fc = tuple(o.fractal_color)
    same = dict(TR.for_scene(name), mid=fc, far=fc)
    got = TR.march(oracle, s, c, o, it, same, LR.A, OR.DEFAULT, _ext(oracle, True))
    assert (got.t[got.hit] > 0).any()
    assert TR.same_bits(got.rgb, want.rgb).all()
    assert (TR.encode(oracle, got.rgb, 1) == LR.encode(oracle, want.rgb, 1)).all()


def test_heatmap_evaluates_no_trap(kifs, oracle):
    screen, cam, gui, iters = cases(kifs, GW, GH)["julia_24"]
    heat = kifs.GuiData(**{**gui.__dict__, "is_heatmap": True, "fractal_color": (255, 128, 30)})
    s, c, o = oracle_uniforms(oracle, kifs, (screen, cam, heat))
    it = oracle.iters(*iters)
    f = TR.march(oracle, s, c, o, it, TR.J, LR.A, OR.DEFAULT, _ext(oracle, True))
    assert (TR.encode(oracle, f.rgb, 1) == oracle.render(s, c, o, it, encode=1, ext=_ext(oracle, True))).all()
    assert f.hit.any() and (f.u == 0).all() and (f.t == 0).all()


def test_u_of_the_sphere_is_the_distance_from_the_origin(kifs, oracle):
    screen, cam, gui, iters = cases(kifs, GW, GH)["sphere"]
    s, c, o = oracle_uniforms(oracle, kifs, (screen, cam, gui))
    spec = dict(TR.S, centre=(0.0, 0.0, 0.0, 0.0), axes=7, iterations=0)
    f = TR.march(oracle, s, c, o, oracle.iters(*iters), spec)
    p = f.pos[f.hit]
    assert len(p) > 100
    want = np.array([np.sqrt(f32(_fma32(q[2], q[2], _fma32(q[1], q[1], _fma32(q[0], q[0], f32(0)))))) for q in p], dtype=f32)
    assert TR.same_bits(f.u[f.hit], want).all()
    assert TR.same_bits(TR.eval_u(oracle, o, spec, p), want).all()
    # ... and with orbit points asked for: a primitive has z_0 only
    assert TR.same_bits(TR.eval_u(oracle, o, dict(spec, iterations=32), p), want).all()
    # one bit is a plane, two a line
    assert TR.same_bits(TR.eval_u(oracle, o, dict(spec, axes=2), p), np.abs(p[:, 1])).all()


def test_the_gradient_at_its_stops(kifs, oracle):
    screen, cam, gui, iters = cases(kifs, GW, GH)["julia_24"]
    _, _, o = oracle_uniforms(oracle, kifs, (screen, cam, gui))
    spec = dict(TR.J, scale=1.0, bias=0.0)
    fc = np.array(list(o.fractal_color), dtype=f32)
    mid, far = np.array(TR.MID, dtype=f32), np.array(TR.FAR, dtype=f32)

    def stop(f, a, b):  # fma(f, b - a, a) per channel
        return np.array([_fma32(f32(f), f32(b[i] - a[i]), a[i]) for i in range(3)], dtype=f32)

    # (the far stop itself is fma(1, far - mid, mid): far to within the rounding of the difference)
    for u, t, want in ((0.0, 0.0, fc), (0.5, 0.5, mid), (1.0, 1.0, stop(1.0, mid, far)), (7.0, 1.0, stop(1.0, mid, far)),
                       (float("inf"), 1.0, stop(1.0, mid, far)), (float("nan"), 0.0, fc), (-3.0, 0.0, fc),
                       (0.25, 0.25, stop(0.5, fc, mid)), (0.875, 0.875, stop(0.75, mid, far))):
        tt, col = TR.colour(oracle, o, spec, u)
        assert tt == f32(t) and TR.same_bits(col, want).all(), (u, tt, col)
    assert np.abs(stop(1.0, mid, far) - far).max() < 1e-7


@pytest.mark.parametrize("name,trap_name", [("julia_24", "J"), ("sierpinski", "S")])
def test_the_test_traps_colour_the_frames(name, trap_name, kifs, oracle):
    """A guard against a GPU test that shows nothing.  (A prototype of the contract gave J: 207 hits, 107 codes, 136 and
    71 hits in the two segments, 3 and 14 saturated; S: 128 hits, 87 codes, 87 and 41 hits.)"""
    screen, cam, gui, iters = cases(kifs, GW, GH)[name]
    f = TR.trapped_frame(oracle, kifs, screen, cam, gui, iters, getattr(TR, trap_name), LR.A)
    t = f.t[f.hit]
    codes = len(np.unique(np.rint(255.0 * t.astype(np.float64))))
    lower, upper = int((t < 0.5).sum()), int((t >= 0.5).sum())
    print(name, "hits", len(t), "codes", codes, "segments", lower, upper, "t = 0:", int((t == 0).sum()), "t = 1:", int((t == 1).sum()))
    assert codes >= 32 and lower >= 10 and upper >= 10
    if trap_name == "J":
        assert (t == 0).any() and (t == 1).any()
    flat = TR.trapped_frame(oracle, kifs, screen, cam, gui, iters, dict(getattr(TR, trap_name), scale=0.0, bias=0.0), LR.A)
    assert not TR.same_bits(f.rgb, flat.rgb).all()
