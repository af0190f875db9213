"""tests/lighting_reference.c IS the contract of kifs_render_lit_async on the oracle.  With the reference's light and no
term its frame is kor_render_ext's, byte for byte, for every pipeline with soft shadows on and off; with the default
occlusion term its colours and factors are tests/occlusion_reference.c's bit for bit; its direct term and its highlight
equal a NumPy f32 restatement with an exactly rounded fma at 240 distinct seeded hits under two lights.  And the scenes
the GPU tests use do exercise the light: under the test light A every pipeline has partially lit pixels, pixels turned away from the light and pixels
with a visible highlight, and A's shadows change some hit pixels of the shadow scenes and leave others.  That is what
makes the GPU comparison of tests/test_gpu_lighting.py mean something.  CPU only."""
import numpy as np
import pytest

import lighting_reference as LR
import occlusion_reference as OR
from geometry_cases import PIPELINES, cases
from helpers import oracle_uniforms
from test_occlusion_reference import _fma32

GW, GH = 102, 45       # the frames of the GPU tests, and of the comparison with kor_render_ext
f32 = np.float32


def _ext(oracle, on):
    return oracle.Ext(1, 64, 8.0, 0.02, 10.0) if on else None  # the soft-shadow block of tests/test_gpu_occlusion.py


_FRAMES = {}


def _frame(oracle, kifs, name, spec_name, ao=None, shadows=False):
    key = (name, spec_name, ao, shadows)
    if key not in _FRAMES:
        screen, cam, gui, iters = cases(kifs, GW, GH)[name]
        _FRAMES[key] = LR.lit_frame(oracle, kifs, screen, cam, gui, iters, getattr(LR, spec_name), ao, _ext(oracle, shadows))
    return _FRAMES[key]


@pytest.mark.parametrize("shadows", [False, True])
@pytest.mark.parametrize("name", PIPELINES)
def test_reference_light_is_the_oracles_frame(name, shadows, kifs, oracle):
    screen, cam, gui, iters = cases(kifs, GW, GH)[name]
    s, c, o = oracle_uniforms(oracle, kifs, (screen, cam, gui))
    it = oracle.iters(*iters)
    f = _frame(oracle, kifs, name, "REFERENCE", shadows=shadows)
    for encode in (1, 0):
        want = oracle.render(s, c, o, it, encode=encode, ext=_ext(oracle, shadows))
        got = LR.encode(oracle, f.rgb, encode)
        assert (got == want).all(), (name, shadows, encode, int((got != want).any(-1).sum()))
    # any shininess: no highlight is computed without a weight
    g = LR.march(oracle, s, c, o, it, dict(LR.REFERENCE, shininess_log2=0), None, _ext(oracle, shadows))
    assert LR.same_bits(g.rgb, f.rgb).all()


@pytest.mark.parametrize("shadows", [False, True])
@pytest.mark.parametrize("name", PIPELINES)
def test_reference_light_with_the_default_term_is_the_occlusion_model(name, shadows, kifs, oracle):
    screen, cam, gui, iters = cases(kifs, GW, GH)[name]
    f = _frame(oracle, kifs, name, "REFERENCE", OR.DEFAULT, shadows)
    want = OR.occlusion_frame(oracle, kifs, screen, cam, gui, iters, OR.DEFAULT, _ext(oracle, shadows))
    assert (f.hit == want.hit).all()
    assert LR.same_bits(f.rgb, want.rgb).all(), (name, shadows)
    assert LR.same_bits(f.a, want.plane).all(), (name, shadows)
    assert LR.same_bits(f.normal, want.normal).all() and LR.same_bits(f.pos, want.pos).all()


def test_heatmap_is_the_counters_colour(kifs, oracle):
    screen, cam, gui, iters = cases(kifs, GW, GH)["julia_24"]
    heat = kifs.GuiData(**{**gui.__dict__, "is_heatmap": True, "fractal_color": (255, 128, 30)})
    s, c, o = oracle_uniforms(oracle, kifs, (screen, cam, heat))
    it = oracle.iters(*iters)
    f = LR.march(oracle, s, c, o, it, LR.A, OR.DEFAULT, _ext(oracle, True))
    assert (LR.encode(oracle, f.rgb, 1) == oracle.render(s, c, o, it, encode=1, ext=_ext(oracle, True))).all()
    assert f.hit.any()


def _dot3(a, b):
    a, b = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32)
    return f32(_fma32(a[2], b[2], _fma32(a[1], b[1], f32(a[0] * b[0]))))


def _normalize3(v):
    v = np.asarray(v, dtype=f32)
    l = f32(np.sqrt(_dot3(v, v)))
    return np.array([f32(v[0] / l), f32(v[1] / l), f32(v[2] / l)], dtype=f32)


def _clamp01(e):
    lo = f32(0) if e < 0 else e
    return f32(1) if 1 < lo else lo


def _highlight_numpy(spec, n, d):
    lh = _normalize3(spec["direction"])
    h = _normalize3(np.array([f32(lh[0] - d[0]), f32(lh[1] - d[1]), f32(lh[2] - d[2])], dtype=f32))
    s = _clamp01(_dot3(n, h))
    for _ in range(spec["shininess_log2"]):
        s = f32(s * s)
    return s


def test_direct_term_and_highlight_equal_the_numpy_restatement(kifs, oracle):
    """240 DISTINCT hits: per scene one seeded shuffle of the hit pixels, the first 30 held under light A, the next 30
    under light B (another direction, other weights, e = 5)."""
    rng = np.random.default_rng(0x11a7)
    seen = set()
    for name in ("julia_24", "sierpinski", "torus", "bunny"):
        screen, cam, gui, iters = cases(kifs, GW, GH)[name]
        s, c, o = oracle_uniforms(oracle, kifs, (screen, cam, gui))
        hits = _frame(oracle, kifs, name, "A")
        ys, xs = np.nonzero(hits.hit & ~np.isnan(hits.normal).any(-1))  # (the hits do not depend on the light)
        order = rng.permutation(len(ys))
        assert len(order) >= 60, name
        for part, spec_name in enumerate(("A", "B")):
            spec = getattr(LR, spec_name)
            assert LR.same_bits(LR.unit(oracle, spec), _normalize3(spec["direction"])).all()
            f = _frame(oracle, kifs, name, spec_name)
            assert (f.hit == hits.hit).all()
            lit, shiny = 0, 0
            for k in order[30 * part:30 * part + 30]:
                y, x = int(ys[k]), int(xs[k])
                n = f.normal[y, x]
                d = np.array(oracle.ray_direction(s, c, x, y), dtype=f32)
                lit0 = _clamp01(_dot3(n, np.asarray(spec["direction"], dtype=f32)))
                hl = _highlight_numpy(spec, n, d)
                assert LR.same_bits(LR.direct(oracle, spec, n), lit0).all() and LR.same_bits(f.lit0[y, x], lit0).all(), (name, spec_name, x, y)
                assert LR.same_bits(LR.highlight(oracle, spec, n, d), hl).all() and LR.same_bits(f.s[y, x], hl).all(), (name, spec_name, x, y)
                # and the colour the frame holds is the contract's, from these terms
                kk = f32(_fma32(f32(spec["diffuse"]), lit0, f32(spec["ambient"])))
                spc = hl if lit0 > 0 else f32(0)
                fc = np.array(list(o.fractal_color), dtype=f32)
                want = np.array([_fma32(f32(spec["specular"][i]), spc, f32(kk * fc[i])) for i in range(3)], dtype=f32)
                assert LR.same_bits(f.rgb[y, x], want).all(), (name, spec_name, x, y)
                seen.add((name, x, y))
                lit += int(lit0 > 0)
                shiny += int(lit0 > 0 and hl > 0)
            print(name, spec_name, "checked 30 hits:", lit, "with a direct term,", shiny, "of them with a highlight")
    assert len(seen) == 240  # distinct (scene, pixel) hits, 120 under each light


@pytest.mark.parametrize("name", [p for p in PIPELINES if p != "unknown_id"])
def test_light_a_exercises_every_branch_of_the_contract(name, kifs, oracle):
    """A guard against a GPU test that shows nothing: at the GPU tests' size, under the test light A (e = 3), every
    pipeline has pixels partially lit, pixels turned away and pixels with a visible highlight.  (An f64 approximation of
    the contract gave as smallest counts 22 (genjulia), 13 (bunny) and 12 (genjulia).)"""
    f = _frame(oracle, kifs, name, "A")
    partial = int((f.hit & (f.lit0 > 0) & (f.lit0 < 1)).sum())
    away = int((f.hit & (f.lit0 == 0)).sum())
    shiny = int((f.hit & (f.lit0 > 0) & (f.s > 0.02)).sum())
    print(name, "hits", int(f.hit.sum()), "0 < lit0 < 1:", partial, "lit0 = 0:", away, "lit0 > 0 and s > 0.02:", shiny)
    assert partial >= 8 and away >= 8 and shiny >= 8
    assert f.hit.any() and not f.hit.all()


def test_the_box_has_no_highlight_pixel_at_e_5(kifs, oracle):
    """... which is why the test light's e is 3."""
    f = _frame(oracle, kifs, "box", "A5")
    assert int((f.hit & (f.lit0 > 0) & (f.s > 0.02)).sum()) == 0


@pytest.mark.parametrize("name", ["julia_24", "sierpinski"])
def test_shadows_towards_a_change_some_hits_and_leave_others(name, kifs, oracle):
    plain = _frame(oracle, kifs, name, "A")
    shadowed = _frame(oracle, kifs, name, "A", shadows=True)
    assert (plain.hit == shadowed.hit).all()
    same = LR.same_bits(plain.rgb, shadowed.rgb).all(-1)
    print(name, "hit pixels the shadows change:", int((plain.hit & ~same).sum()), "and leave:", int((plain.hit & same).sum()))
    assert (plain.hit & ~same).any() and (plain.hit & same).any()
    assert same[~plain.hit].all()
    # a shadow ray is marched only where there is a direct term
    assert (shadowed.sh[shadowed.hit & ~(shadowed.lit0 > 0)] == 1.0).all()
