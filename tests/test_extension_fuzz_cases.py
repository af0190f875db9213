"""The scenes of tests/extension_fuzz_cases.py held to the oracle and the reference helpers alone, so that the GPU
families built on them cannot pass on empty frames: most scenes show hits and misses and have edge pixels at the
thresholds the adaptive family uses for them, every pipeline does so from two camera families, the short marches, the
heatmaps and the all-background unknown primitive are there, the cameras are where the families say, and the scenes reach
all ten (GROUP, PRIM) instantiations.  Conditions, not measurements: if a seed misses one, change the seed or the ranges.
CPU only; the product renders nothing here."""
import numpy as np
import pytest

import adaptive_reference as AR
import extension_fuzz_cases as X
import extension_fuzz_support as S
from geometry_cases import PIPELINES, Raw
from helpers import oracle_frame

KNOWN = [i for i in range(X.N) if PIPELINES[i % 10] != "unknown_id"]


@pytest.fixture(scope="module")
def facts(oracle, kifs):
    """Per scene: (hit mask, edge mask at the scene's thresholds)."""
    out = []
    for i in range(X.N):
        geom, hit = S.geometry(oracle, kifs, i)
        out.append((hit, AR.edge_mask(geom, *X.thresholds(i))))
    return out


def _both(hit):
    return bool(hit.any() and not hit.all())


def test_seeded_and_shaped_as_the_families_expect(kifs):
    a, b = X.scenes(kifs), list(X._scenes.__wrapped__(kifs, X.N, X.SEED))
    assert len(a) == X.N >= 36
    for i, (s, t) in enumerate(zip(a, b)):
        name, family, screen, cam, gui, iters, encode = s
        assert name == PIPELINES[i % 10] == t[0] and family == X.family_of(i) == t[1] and encode in (0, 1)
        assert (screen, cam, iters, encode) == (t[2], t[3], t[5], t[6])
        assert kifs.uniform_bytes(gui.into_buffer_data()) == kifs.uniform_bytes(t[4].into_buffer_data())
        heavy = name in X.HEAVY
        assert 17 <= screen.width <= (56 if heavy else 96) and 9 <= screen.height <= (40 if heavy else 72)
        g = X.options_of(gui)
        assert 1 <= g.max_iterations <= (50 if heavy else 400) and (g.max_iterations <= 3) == X.is_short_march(i)
        assert 10 <= g.max_distance <= 1e4 and 1e-5 <= g.epsilon <= 1e-1 and 1 <= g.power <= 10
        assert all(-1 <= c <= 1 for c in g.constant) and g.is_heatmap == X.is_heatmap(i)
        assert isinstance(gui, Raw) == (name == "unknown_id")
        if name == "unknown_id":
            assert gui.u.primitive_id == 17
        lo, hi = {"julia_24": (1, 24), "julia_25": (25, 40), "genjulia": (1, 7)}.get(name, (0, 39))
        assert lo <= iters[0] <= hi and 0 <= iters[1] <= (3 if heavy else 11) and 0 <= iters[2] <= 23
        # the camera against the two cull radii of its scene
        r = cam.origin_distance / X.radius(name, gui)
        assert cam.min_distance == 0.05 and abs(cam.theta) <= 1.5 and 0 <= cam.phi <= 2 * np.pi
        assert [0.5 <= r <= 0.95, r == 1.0, np.sqrt(1.1) < 1.05 <= r <= 1.09 < np.sqrt(1.2), np.sqrt(1.2) < 1.10 <= r <= 2.5][family], (i, r)


def test_every_pipeline_meets_every_family_and_every_threshold_kind():
    for p in range(10):
        mine = [i for i in range(X.N) if i % 10 == p]
        assert {X.family_of(i) for i in mine} == {0, 1, 2, 3}
        kinds = [X.thresholds(i) for i in mine]
        assert sum(t in (AR.SILHOUETTE, AR.DEFAULT, AR.ALL_HITS) for t in kinds) == 3 and len(set(kinds)) == 4
    for i in range(X.N):
        assert X.family_of(i) not in X.other_families(i) and len(set(X.other_families(i))) == 2


def test_sizes_fall_on_both_sides_of_the_kernels_strides(kifs):
    sizes = [(s[2].width, s[2].height) for s in X.scenes(kifs)]
    w, h = np.array(sizes).T
    assert (w < 64).any() and (w > 64).any() and (h < 64).any() and (h > 64).any()
    assert (w % 32 != 0).sum() > X.N // 2 and (h % 8 != 0).sum() > X.N // 2           # most are ragged
    assert (w % 32 == 0).any() and (h % 8 == 0).any()
    low = [i for i in range(X.N) if sizes[i][1] < 4 * X.supersampling(i)]             # lower than 4 k rows
    assert len(low) >= 3 and {X.supersampling(i) for i in low} == {3, 4}


def test_hits_and_misses(facts):
    both = [i for i in KNOWN if _both(facts[i][0])]
    print("hit-and-miss scenes:", len(both), "of", len(KNOWN), "; all-hit:", sum(bool(facts[i][0].all()) for i in KNOWN),
          "; no-hit:", sum(not facts[i][0].any() for i in KNOWN))
    assert 3 * len(both) >= 2 * len(KNOWN), both


def test_edges(facts):
    edged = [i for i in KNOWN if facts[i][1].any() and int(facts[i][1].sum()) % 7 != 0]
    print("scenes with an edge mask of a size no multiple of 7:", len(edged), "of", len(KNOWN))
    assert 3 * len(edged) >= 2 * len(KNOWN), edged


def test_per_pipeline(facts):
    for p, name in enumerate(PIPELINES):
        if name == "unknown_id":
            continue
        both = [i for i in range(p, X.N, 10) if _both(facts[i][0])]
        assert len(both) >= 2 and len({X.family_of(i) for i in both}) >= 2, (name, both)


def test_per_family(facts):
    """(Not a condition of its own beyond presence: every family shows hits and misses somewhere.)"""
    per = {f: [i for i in KNOWN if X.family_of(i) == f and _both(facts[i][0])] for f in range(4)}
    print("hit-and-miss scenes per camera family:", {f: len(v) for f, v in per.items()})
    assert all(per.values())


def test_short_marches(kifs, facts):
    short = [i for i in range(X.N) if X.is_short_march(i)]
    assert len(short) >= 4
    assert {X.options_of(X.scenes(kifs)[i][4]).max_iterations for i in short} <= {1, 2, 3}


def test_heatmaps(kifs, oracle, facts):
    heat = [i for i in range(X.N) if X.is_heatmap(i)]
    hitting = [i for i in heat if facts[i][0].any()]
    assert len(hitting) >= 3, hitting
    # and a heatmap frame is not the shaded frame's bytes
    i = hitting[0]
    _, _, screen, cam, gui, iters, encode = X.scenes(kifs)[i]
    shaded = kifs.GuiData(**{**X.options_of(gui).__dict__, "is_heatmap": False})
    assert (oracle_frame(oracle, kifs, screen, cam, gui, iters, encode=encode)
            != oracle_frame(oracle, kifs, screen, cam, X.pack(kifs, PIPELINES[i % 10], shaded), iters, encode=encode)).any()


def test_unknown_id_is_all_background(kifs, oracle, facts):
    for i in range(9, X.N, 10):
        _, _, screen, cam, gui, iters, encode = X.scenes(kifs)[i]
        assert not facts[i][0].any() and not facts[i][1].any()
        f = oracle_frame(oracle, kifs, screen, cam, gui, iters, encode=encode)
        assert (f == f[0, 0]).all()


def test_instantiations(kifs):
    reached = {}
    for name, _, _, _, gui, iters, _ in X.scenes(kifs):
        reached.setdefault(X.dispatch(name, gui, iters), set()).add(name)
    assert sorted(reached) == [(0, p) for p in range(7)] + [(1, 0), (1, 1), (2, 0)]
    assert all(len(v) == 1 for v in reached.values())  # one pipeline name per instantiation, as kernel_forms claims them
    assert reached[(1, 1)] == {"julia_24"} and reached[(1, 0)] == {"julia_25"} and reached[(0, 6)] == {"unknown_id"}


def test_soft_shadow_scenes(kifs, oracle, facts):
    """The scenes the families run with the extension on: not heatmaps, with hits, and in some of them a secondary ray
    meets the fractal (the oracle's frame with the extension differs from the one without)."""
    on = [i for i in range(X.N) if X.shadow_candidate(i) is not None and facts[i][0].any()]
    assert len(on) >= 5
    changed = 0
    for i in on:
        _, _, screen, cam, gui, iters, encode = X.scenes(kifs)[i]
        sh = X.shadow_candidate(i)
        assert 4 <= sh["shadow_steps"] <= 32 and 2 <= sh["shadow_k"] <= 16 and 0.005 <= sh["shadow_t0"] <= 0.05 \
            and 2 <= sh["shadow_max_t"] <= 8 and not X.is_heatmap(i)
        from helpers import oracle_uniforms
        s, c, o = oracle_uniforms(oracle, kifs, (screen, cam, gui))
        plain = oracle.render(s, c, o, oracle.iters(*iters), encode=encode)
        changed += int((oracle.render(s, c, o, oracle.iters(*iters), encode=encode, ext=X.oracle_ext(oracle, sh)) != plain).any())
    print("soft-shadow scenes:", on, "; the extension changes", changed)
    assert changed >= 3


def test_animation_sequences(kifs):
    zeros = 0
    for i, scene in enumerate(X.scenes(kifs)):
        screen, frames, lone = X.animation(kifs, i, scene)
        assert len(frames) == (2, 5, 9)[i % 3] and 0 <= lone < len(frames)
        assert screen.width <= 64 and screen.height <= 48
        images = [g.into_buffer_data() for _, g in frames]
        for u in images[1:]:  # only constant, power and the colours differ between the frames of a launch
            for f in ("max_iterations", "max_distance", "epsilon", "is_heatmap", "fractal_group_id", "primitive_id"):
                assert getattr(u, f) == getattr(images[0], f)
        if i % 3 == 1:
            bits = [np.array(list(u.constant), dtype=np.float32).view(np.uint32) for u in images]
            assert sum((b == 0).any() for b in bits) == 1 and sum((b == 0x80000000).any() for b in bits) == 1
            zeros += 1
    assert zeros >= 12


def test_batches_reach_every_pipeline_and_every_k():
    """The 3-view batches of the supersampling, geometry and adaptive families, and the geometry family's bands."""
    batches = [i for i in range(X.N) if X.has_batch(i)]
    assert X.N // 3 <= len(batches) <= X.N // 3 + 2
    assert {i % 10 for i in batches} == set(range(10)), "a pipeline without a batch"
    assert {X.supersampling(i) for i in batches} == {2, 3, 4}
    assert len({X.family_of(i) for i in batches}) == 4
    assert [X.batch_number(i) for i in batches] == list(range(len(batches)))
    bands = [i for i in batches if X.has_band(i)]
    known = [i % 10 for i in bands if PIPELINES[i % 10] != "unknown_id"]
    assert len(bands) == (len(batches) + 1) // 2 and len(set(known)) >= 5, bands
    assert sum(known.count(p) >= 2 for p in set(known)) >= 2, bands   # and two pipelines meet two bands each
    shadowed = [i for i in batches if X.shadow_candidate(i) is not None]
    assert len(shadowed) >= 3, shadowed


def test_batches_show_hits_and_misses(facts):
    """At least two thirds of the known pipelines' batch scenes show hits and misses from the scene's own camera."""
    batches = [i for i in KNOWN if X.has_batch(i)]
    both = [i for i in batches if _both(facts[i][0])]
    print("batch scenes with hits and misses:", len(both), "of", len(batches))
    assert 3 * len(both) >= 2 * len(batches), both


def test_resolve_with_the_extension_is_the_oracles_frame_at_k1(kifs, oracle, facts):
    """kor_shade_pixel_ext, which the supersampling and adaptive references resolve soft-shadow scenes from, shades what
    kor_render_ext encodes: at k = 1 the resolve is the oracle's own frame with the extension, and differs from the one
    without it."""
    import aa_reference as AA
    i = next(i for i in range(X.N) if X.shadow_candidate(i) is not None and _both(facts[i][0]))
    _, _, screen, cam, gui, iters, encode = X.scenes(kifs)[i]
    shadow = X.shadow_candidate(i)
    for enc in (0, 1):
        with_ext = AA.aa_frame(oracle, kifs, screen, cam, gui, iters, 1, enc, ext=X.oracle_ext(oracle, shadow))
        assert (with_ext == S.expected_colour(oracle, kifs, screen, cam, gui, iters, enc, shadow)).all()
        assert (AA.aa_frame(oracle, kifs, screen, cam, gui, iters, 1, enc) == oracle_frame(oracle, kifs, screen, cam, gui, iters, encode=enc)).all()
    assert (with_ext != oracle_frame(oracle, kifs, screen, cam, gui, iters, encode=1)).any()
