"""The draws of tests/shading_fuzz_cases.py held to the models alone (tests/lighting_reference.c,
tests/occlusion_reference.c and the oracle), so that the GPU families built on them cannot pass with the light or the
term unseen: per pipeline the fuzzed lights leave pixels partially lit, a highlight that changes bytes and partial
factors; over the family there are clamped factors, shadowed pixels, a visible highlight at every shininess, hits under
every class of direction length, channels past 1.0 before the encode and a lone channel of every colour that shows.  And
the models are held to the oracle on these scenes -- a camera inside the set, marches of 1-3 steps, the unknown primitive
--, where tests/test_lighting_reference.py holds them at hand-picked hits.  Conditions, not measurements: if a salt
misses one, change the salt or the ranges, never the condition.  Every test prints its counts.  CPU only."""
import numpy as np
import pytest

import extension_fuzz_cases as X
import extension_fuzz_support as S
import lighting_reference as LR
import occlusion_reference as OR
import shading_fuzz_cases as Z
from geometry_cases import PIPELINES
from helpers import oracle_uniforms

KNOWN = [i for i in range(X.N) if PIPELINES[i % 10] != "unknown_id"]
NAMED = [p for p in PIPELINES if p != "unknown_id"]


class Facts:
    """Per scene: the lit model's frame (with the family's term or None), the same without a highlight, without the
    term, the occlusion model's frame with term(i), and the oracle's plain frame, with the scene's encode and shadows."""


@pytest.fixture(scope="module")
def facts(oracle, kifs):
    O, K = oracle, kifs
    out = []
    for i, (name, _, screen, cam, gui, iters, encode) in enumerate(X.scenes(K)):
        f = Facts()
        f.shadow = S.shadow_of(O, K, i)
        f.ext = X.oracle_ext(O, f.shadow)
        f.encode = encode
        f.spec, f.term = Z.light(i), Z.lit_term(i)
        scene = (screen, cam, gui, iters)
        f.lit = LR.lit_frame(O, K, *scene, f.spec, f.term, f.ext)
        f.dull = LR.lit_frame(O, K, *scene, dict(f.spec, specular=(0.0, 0.0, 0.0)), f.term, f.ext)
        f.bare = f.lit if f.term is None else LR.lit_frame(O, K, *scene, f.spec, None, f.ext)
        f.occluded = OR.occlusion_frame(O, K, *scene, Z.term(i), f.ext)
        f.plain = S.expected_colour(O, K, *scene, encode, f.shadow)
        f.bytes = LR.encode(O, f.lit.rgb, encode)
        out.append(f)
    return out


def _of(p):
    return range(p, X.N, 10)


def test_the_draws_are_what_the_families_are_told(kifs):
    lights, terms = [Z.light(i) for i in range(Z.N)], [Z.term(i) for i in range(Z.N)]
    assert lights == [Z.light(i) for i in range(Z.N)] and Z.N == X.N == len(X.scenes(kifs))
    classes = [Z.scale_class(i) for i in range(Z.N)]
    assert (classes.count(Z.UNIT), classes.count(Z.SMALL), classes.count(Z.LARGE)) == (24, 8, 8)
    for i, l in enumerate(lights):
        d = np.array(l["direction"], dtype=np.float32)
        # dot3 as light_ok takes it is a normal f32 for every class, with a factor of eight to spare at either end
        d2 = float((d.astype(np.float64) ** 2).sum())
        assert np.isfinite(d).all() and 1e-37 < d2 < 1e37, (i, d2)
        n = float(np.linalg.norm(d.astype(np.float64)))
        lo, hi = {Z.UNIT: (0.9999999, 1.0000001), Z.SMALL: (0.99e-18, 1.01e-2), Z.LARGE: (9.9, 1.01e18)}[classes[i]]
        assert lo <= n <= hi, (i, n)
        assert 0 <= l["ambient"] <= 0.5 and 0 <= l["diffuse"] <= 1.5 and all(0 <= s <= 1 for s in l["specular"])
        assert l["shininess_log2"] == i % 11
        lone = Z.one_channel(i)
        assert (sum(s != 0 for s in l["specular"]) == 0) == (i % 4 == 3)
        assert lone is None or [s != 0 for s in l["specular"]] == [c == lone for c in range(3)]
    assert sum(l["ambient"] == 0 for l in lights) >= 2 and sum(l["diffuse"] == 0 for l in lights) >= 2
    assert sum(l["diffuse"] > 1 for l in lights) >= 4
    lone = [Z.one_channel(i) for i in range(Z.N) if Z.one_channel(i) is not None]
    assert len(lone) >= 3 and set(lone) == {0, 1, 2}
    for samples, step, decay, strength in terms:
        assert 1 <= samples <= 16 and 1e-3 <= step <= 10 ** -0.5 and 0.3 <= decay <= 1 and 0 <= strength <= 8
    assert sum(t[0] == 1 for t in terms) >= 2 and sum(t[0] == 16 for t in terms) >= 2
    assert sum(t[2] == 1.0 for t in terms) >= 2 and sum(t[3] == 0.0 for t in terms) == 1
    carried = [Z.lit_term(i) is not None for i in range(Z.N)]
    assert carried.count(False) == Z.N // 3 and all(Z.lit_term(i) in (None, terms[i]) for i in range(Z.N))
    print("ambient 0:", [i for i, l in enumerate(lights) if l["ambient"] == 0], "; diffuse 0:",
          [i for i, l in enumerate(lights) if l["diffuse"] == 0], "; diffuse > 1:", sum(l["diffuse"] > 1 for l in lights),
          "; one channel:", len(lone), "; 1 probe:", [i for i, t in enumerate(terms) if t[0] == 1], "; 16 probes:",
          [i for i, t in enumerate(terms) if t[0] == 16], "; decay 1:", [i for i, t in enumerate(terms) if t[2] == 1.0])


def test_batches_meet_every_arrangement(kifs):
    batches = [i for i in range(X.N) if X.has_batch(i)]
    planes = [i for i in batches if Z.occlusion_batch_has_plane(i)]
    bands = [i for i in batches if X.has_band(i)]
    print("batches:", batches, "; bands:", bands, "; occlusion batches at k = 1 with a plane:", planes)
    assert len(batches) >= 12 and 2 * len(planes) in (len(batches) - 1, len(batches), len(batches) + 1)
    assert set(planes) & set(bands) and set(planes) - set(bands) and set(bands) - set(planes)
    assert {Z.occlusion_batch_k(i) for i in batches if i not in planes} >= {2, 3} and {Z.occlusion_batch_k(i) for i in planes} == {1}
    assert any(Z.lit_term(i) is None for i in batches) and sum(Z.lit_term(i) is not None for i in batches) >= 6
    for i in bands:
        h = X.scenes(kifs)[i][2].height
        for salt in (Z.LIT_BATCH_SALT, Z.OCCLUSION_BATCH_SALT):
            y0, y1 = Z.band(i, h, salt)
            assert 0 < y0 < y1 <= h and y0 % 8 and y1 % 8
    assert all(Z.band(i, 40, 1) == (0, 40) for i in batches if i not in bands)


def _changed_by_highlight(f, O):
    return (LR.encode(O, f.lit.rgb, f.encode) != LR.encode(O, f.dull.rgb, f.encode)).any(-1)


def test_per_pipeline(facts, oracle):
    """Two scenes with 8 or more partially lit hit pixels per pipeline -- where the family's scenes have two with 8 hit
    pixels at all.  The generalised Julia set's four have 280, 1, 0 and 3 hit pixels (scenes 2, 12, 22, 32: the scenes
    and their seed are tests/extension_fuzz_cases.py's, shared with four other families, and no draw of a light makes a
    pixel hit), so one scene is all it can have; every other pipeline must have two, and the exception is pinned."""
    enough = {name: sum(int(facts[i].lit.hit.sum()) >= 8 for i in _of(p)) for p, name in enumerate(PIPELINES)}
    assert {name for name in NAMED if enough[name] < 2} == {"genjulia"} and enough["genjulia"] == 1, enough
    for p, name in enumerate(PIPELINES):
        if name == "unknown_id":
            continue
        heat = [i for i in _of(p) if X.is_heatmap(i)]
        partial = {i: int((facts[i].lit.hit & (facts[i].lit.lit0 > 0) & (facts[i].lit.lit0 < 1)).sum()) for i in _of(p)}
        highlit = {i: int(_changed_by_highlight(facts[i], oracle).sum()) for i in _of(p)}
        occluded = {i: int((facts[i].occluded.hit & (facts[i].occluded.plane > 0) & (facts[i].occluded.plane < 1)).sum()) for i in _of(p)}
        print(f"{name}: pixels partially lit {partial}; pixels whose bytes the highlight changes {highlit}; "
              f"pixels with a partial factor {occluded}; heatmaps {heat}")
        assert sum(v >= 8 for v in partial.values()) >= min(2, enough[name]), (name, partial)
        assert any(highlit.values()), (name, highlit)
        assert any(occluded.values()), (name, occluded)


def test_over_the_family(facts, oracle):
    clamped = {i: int((f.occluded.hit & (f.occluded.plane == 0)).sum()) for i, f in enumerate(facts)}
    print("hit pixels with a factor of 0:", {i: v for i, v in clamped.items() if v})
    assert max(clamped.values()) >= 20
    shadowed = {i: int((f.lit.hit & (f.lit.sh < 1)).sum()) for i, f in enumerate(facts)}
    shadowed = {i: v for i, v in shadowed.items() if v}
    print("hit pixels with sh < 1:", shadowed)
    assert len(shadowed) >= 3 and len({i % 10 for i in shadowed}) >= 3
    per_e = {e: [i for i, f in enumerate(facts) if i % 11 == e and (f.lit.hit & (f.lit.lit0 > 0) & (f.lit.s > 0)).any()] for e in range(11)}
    print("scenes with s > 0 on a lit hit pixel, per shininess_log2:", per_e)
    assert all(per_e.values())
    per_class = {c: [i for i, f in enumerate(facts) if Z.scale_class(i) == c and f.lit.hit.any()] for c in (Z.UNIT, Z.SMALL, Z.LARGE)}
    print("scenes with hits per class of direction length (unit, short, long):", {c: len(v) for c, v in per_class.items()})
    assert all(per_class.values())
    # a short direction leaves the direct term near 0 and a long one at 0 or 1: the unit vector is in use elsewhere
    assert all((facts[i].lit.lit0[facts[i].lit.hit] < 0.02).all() for i in per_class[Z.SMALL])
    assert any((facts[i].lit.lit0[facts[i].lit.hit] == 1).any() for i in per_class[Z.LARGE])
    bright = [i for i in KNOWN if not X.is_heatmap(i) and (facts[i].lit.rgb[facts[i].lit.hit] > 1.0).any()]
    print("scenes with a linear channel above 1.0 before the encode:", bright)
    assert bright
    channels = {Z.one_channel(i) for i in KNOWN if Z.one_channel(i) is not None and _changed_by_highlight(facts[i], oracle).any()}
    print("lone specular channels whose highlight changes bytes:", sorted(channels))
    assert channels == {0, 1, 2}


def test_the_light_and_the_term_show(facts, oracle):
    """In two thirds of the shaded scenes with hits the lit bytes are not the plain frame's and, where the scene carries
    a term, not the bytes without the term either.  (A term shows only where a probe meets the solid again: the convex
    primitives at small steps have every factor 1.)"""
    scenes = [i for i in KNOWN if facts[i].lit.hit.any() and not X.is_heatmap(i)]
    lit = [i for i in scenes if (facts[i].bytes != facts[i].plain).any()]
    carried = [i for i in scenes if facts[i].term is not None]
    attenuated = [i for i in carried if (facts[i].bytes != LR.encode(oracle, facts[i].bare.rgb, facts[i].encode)).any()]
    shown = [i for i in lit if i not in carried or i in attenuated]
    print("shaded scenes with hits:", len(scenes), "; the light changes the bytes of", len(lit), "; a term is carried in",
          len(carried), "and changes the bytes of", len(attenuated), "; both, or the light alone where there is no term:", len(shown))
    assert 3 * len(shown) >= 2 * len(scenes), (shown, scenes)
    heat = [i for i in range(X.N) if X.is_heatmap(i)]
    assert len(heat) >= 4 and any(facts[i].lit.hit.any() for i in heat)
    for i in heat:  # the contract: a heatmap's colour is the counter's, unlit and unattenuated
        assert (facts[i].bytes == facts[i].plain).all(), i


def test_the_models_are_the_oracle_on_these_scenes(facts, oracle, kifs):
    """lit_frame with the reference's light is kor_render_ext's frame, with term(i) the occlusion model's, and the
    occlusion model without strength the plain frame: on all 40 scenes, both encodes."""
    O, K = oracle, kifs
    hits = shadows = 0
    for i, (name, _, screen, cam, gui, iters, _) in enumerate(X.scenes(K)):
        f = facts[i]
        scene = (screen, cam, gui, iters)
        s, c, o = oracle_uniforms(O, K, (screen, cam, gui))
        ref = LR.lit_frame(O, K, *scene, LR.REFERENCE, None, f.ext)
        with_term = LR.lit_frame(O, K, *scene, LR.REFERENCE, Z.term(i), f.ext)
        samples, step, decay, _ = Z.term(i)
        weak = OR.occlusion_frame(O, K, *scene, (samples, step, decay, 0.0), f.ext)
        for encode in (1, 0):
            want = O.render(s, c, o, O.iters(*iters), encode=encode, ext=f.ext)
            assert (LR.encode(O, ref.rgb, encode) == want).all(), (i, name, encode)
            assert (OR.encode(O, weak.rgb, encode) == want).all(), (i, name, encode)
            assert (LR.encode(O, with_term.rgb, encode) == OR.encode(O, f.occluded.rgb, encode)).all(), (i, name, encode)
        assert (with_term.hit == f.occluded.hit).all() and (ref.hit == f.lit.hit).all()
        assert LR.same_bits(with_term.rgb, f.occluded.rgb).all() and LR.same_bits(with_term.a, f.occluded.plane).all(), (i, name)
        assert (weak.plane == 1).all()
        hits += int(f.lit.hit.sum())
        shadows += f.ext is not None
    print("hit pixels over the 40 scenes:", hits, "; scenes with the soft-shadow extension:", shadows)
    assert shadows >= 5
