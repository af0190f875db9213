"""tests/occlusion_reference.c IS the contract of kifs_render_occlusion_async on the oracle: with strength 0 its frame
is kor_render_ext's, byte for byte, for every pipeline with soft shadows on and off; its march is
tests/geometry_reference.c's; its factor equals a NumPy f32 restatement at seeded hit points; and the scenes the GPU
tests use do exercise the term -- creased surfaces have pixels strictly between 0 and 1 and pixels clamped to 0, convex
primitives have none.  That is what makes the GPU comparison of tests/test_gpu_occlusion.py mean something.  CPU only."""
import numpy as np
import pytest

import geometry_reference as GR
import occlusion_reference as OR
from geometry_cases import PIPELINES, cases
from helpers import oracle_uniforms

W, H = 75, 46          # the frames held to kor_render_ext
GW, GH = 102, 45       # the frames of the GPU tests


def _ext(oracle, on):
    return oracle.Ext(1, 64, 8.0, 0.02, 10.0) if on else None


@pytest.mark.parametrize("shadows", [False, True])
@pytest.mark.parametrize("name", PIPELINES)
def test_strength_zero_is_the_oracles_frame(name, shadows, kifs, oracle):
    screen, cam, gui, iters = cases(kifs, W, H)[name]
    s, c, o = oracle_uniforms(oracle, kifs, (screen, cam, gui))
    it = oracle.iters(*iters)
    ext = _ext(oracle, shadows)
    f = OR.march(oracle, s, c, o, it, (5, 0.02, 0.75, 0.0), ext)
    for encode in (1, 0):
        want = oracle.render(s, c, o, it, encode=encode, ext=ext)
        got = OR.encode(oracle, f.rgb, encode)
        assert (got == want).all(), (name, shadows, encode, int((got != want).any(-1).sum()))
    if not shadows:  # the march is geometry_reference's: the same hits, the same normals
        geom, hit, _ = GR.march(oracle, s, c, o, it)
        assert (f.hit == hit).all()
        assert GR.same_bits(f.normal[hit], geom[hit][:, :3]).all()
        # a factor of 1 - 0 * occ is 1 unless occ is not finite (the generalised Julia set's NaN normals)
        assert ((f.plane == 1.0) | np.isnan(f.plane)).all() and (f.plane[~hit] == 1.0).all()


def _fma32(a, b, c):
    """fma(a, b, c) of f32 values, correctly rounded: the product is exact in f64, the sum is rounded to odd there
    (TwoSum's error term says on which side the exact value lies), and 53 bits round to 24 without a second error."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    prod = a * b
    s = prod + c
    bb = s - prod
    err = (prod - (s - bb)) + (c - bb)
    inexact = np.isfinite(s) & np.isfinite(err) & (err != 0)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    return np.where(inexact & even, np.nextafter(s, toward), s).astype(np.float32)


def _factor_numpy(oracle, o, it, ao, p, n):
    samples, step, decay, strength = ao
    f32 = np.float32
    occ, w = f32(0), f32(1)
    for i in range(1, samples + 1):
        h = f32(step) * f32(i)
        q = _fma32([h, h, h], n, p)
        d = f32(oracle.scene_sdf(o, it, [float(v) for v in q]))
        occ = f32(occ + f32(w * f32(h - d)))
        w = f32(w * f32(decay))
    e = f32(f32(1) - f32(f32(strength) * occ))
    lo = f32(0) if e < 0 else e
    return f32(1) if 1 < lo else lo


_FRAMES = {}


def _frame(oracle, kifs, name, ao):
    key = (name, ao)
    if key not in _FRAMES:
        screen, cam, gui, iters = cases(kifs, GW, GH)[name]
        _FRAMES[key] = OR.occlusion_frame(oracle, kifs, screen, cam, gui, iters, ao)
    return _FRAMES[key]


def test_fma_restatement_is_exact():
    """The cases a double rounding would get wrong: a sum one f64 ulp off an f32 midpoint."""
    one, tiny = np.float32(1), np.float32(2.0 ** -60)
    half_ulp = np.float32(2.0 ** -24)  # 1 + 2^-24 is the midpoint of 1 and 1 + 2^-23
    assert _fma32(half_ulp, one, one) == np.float32(1)                             # the tie goes to even
    assert _fma32(tiny, tiny, np.float32(1) + np.float32(0)) == np.float32(1)
    up = np.float32(np.float64(half_ulp) * (1 + 2.0 ** -23))                       # a hair above the midpoint
    assert _fma32(up, one, one) == np.nextafter(np.float32(1), np.float32(2))
    assert _fma32(np.float32(3), np.float32(5), np.float32(-15)) == 0
    # (2^-12 + 2^-35)(2^-12 - 2^-35) = 2^-24 - 2^-70: with c = 1 + 2^-23 the exact sum is a hair BELOW the midpoint of c
    # and its successor; rounded to f64 first it sits on the midpoint and the tie would go up to the even neighbour
    a, b = np.float32(2.0 ** -12 + 2.0 ** -35), np.float32(2.0 ** -12 - 2.0 ** -35)
    c = np.nextafter(np.float32(1), np.float32(2))
    assert np.float64(a) * np.float64(b) == 2.0 ** -24 - 2.0 ** -70
    assert _fma32(a, b, c) == c and np.float32(np.float64(a) * np.float64(b) + np.float64(c)) != c


@pytest.mark.parametrize("ao", [OR.DEFAULT, OR.DEEP])
def test_factor_equals_the_numpy_restatement(ao, kifs, oracle):
    rng = np.random.default_rng(0x0cc1)
    checked = 0
    for name in ("julia_24", "sierpinski", "torus", "bunny"):
        screen, cam, gui, iters = cases(kifs, GW, GH)[name]
        _, _, o = oracle_uniforms(oracle, kifs, (screen, cam, gui))
        it = oracle.iters(*iters)
        f = _frame(oracle, kifs, name, ao)
        ys, xs = np.nonzero(f.hit)
        for k in rng.choice(len(ys), size=25, replace=False):
            y, x = ys[k], xs[k]
            want = _factor_numpy(oracle, o, it, ao, f.pos[y, x], f.normal[y, x])
            got = OR.factor(oracle, o, it, ao, f.pos[y, x], f.normal[y, x])
            assert OR.same_bits(got, want).all(), (name, x, y, got, want)
            assert OR.same_bits(f.plane[y, x], want).all(), (name, x, y)
            checked += 1
    assert checked == 100  # (two terms: 200 points)


@pytest.mark.parametrize("name", ["julia_24", "julia_25", "genjulia", "sierpinski", "bunny"])
def test_creased_scenes_have_partial_factors(name, kifs, oracle):
    """A guard against a GPU test that shows nothing: at the GPU tests' size and term the scene has pixels whose factor
    is strictly between 0 and 1 (a NumPy prototype with an unfused hit position gave 207, 305, 64, 127 and 47)."""
    f = _frame(oracle, kifs, name, OR.DEFAULT)
    partial = f.hit & (f.plane > 0) & (f.plane < 1)
    print(name, "partial factors:", int(partial.sum()), "of", int(f.hit.sum()), "hits")
    assert int(partial.sum()) >= 32
    assert (f.plane[~f.hit] == 1.0).all()


@pytest.mark.parametrize("name", ["sphere", "box", "torus"])
def test_convex_primitives_are_not_occluded(name, kifs, oracle):
    f = _frame(oracle, kifs, name, OR.DEFAULT)
    assert f.hit.any() and (f.plane[f.hit] == 1.0).all()


@pytest.mark.parametrize("name", ["julia_24", "sierpinski"])
def test_deep_term_clamps_creases_to_zero(name, kifs, oracle):
    """(16, 0.01, 1.0, 1.0): the prototype gave 128 and 33 pixels at 0."""
    f = _frame(oracle, kifs, name, OR.DEEP)
    zero = f.hit & (f.plane == 0)
    print(name, "factors clamped to 0:", int(zero.sum()))
    assert int(zero.sum()) >= 20
