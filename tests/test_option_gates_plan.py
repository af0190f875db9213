"""The gate table of tests/option_gates.py, checked on the CPU with the oracle alone: every gate has a case on each side
by gate_sides(), every case keeps the caps that make its launches short, every case shows what the table says it shows
-- so that a GPU comparison of it is not a comparison of two empty frames --, and expected_tuple() agrees with the
numbers the CPU driver pins (tests/hip_stub/host_driver.cpp, SHAPE_CASES) for the march-budget cases."""
import numpy as np
import pytest

import kernel_forms as F
import lighting_reference as LR
import occlusion_reference as OR
import option_gates as G

W, H = 96, 64
MIN_SHARE, MIN_COLOURS = 0.01, 8


def _frames(O, K, name):
    s = G.SCENES[name]
    ub = K.uniform_bytes
    screen = O.from_bytes(O.Screen, ub(K.ScreenData(W, H).into_buffer_data()))
    options = O.from_bytes(O.Options, ub(G.options(K, name)))
    return [O.render(screen, O.from_bytes(O.Camera, ub(G.camera(K, name, c).into_buffer_data())), options,
                     O.iters(*s.iters), encode=1) for c in range(len(G.CAMERAS))]


def shown(O, K, name):
    """(largest share of pixels of one view that differ from the frame's encoded background, distinct colours over the
    four views).  The background is the far view's corner pixel, as in tests/test_gpu_kernel_forms.py; a heatmap's
    background is its zero-step colour, found the same way."""
    frames = _frames(O, K, name)
    background = frames[-1][0, 0]
    share = max(float((f != background).any(-1).mean()) for f in frames)
    colours = len(np.unique(np.concatenate([f.reshape(-1, 4) for f in frames]), axis=0))
    return share, colours


def test_every_gate_has_a_case_on_each_side():
    sides = {n: G.gate_sides(s) for n, s in G.SCENES.items()}
    of = lambda gate, pred: [n for n in G.names(gate) if pred(G.SCENES[n], *sides[n])]
    # E: the culls go at epsilon < 0 or NaN, the rounds at !(epsilon > 0)
    assert of("E", lambda s, cull, q, t, x2, r: cull and r > 0) and of("E", lambda s, cull, q, t, x2, r: cull and r == 0)
    assert of("E", lambda s, cull, q, t, x2, r: not cull and r == 0)
    # R, D: `sane`, on both pipelines each
    for gate in "RD":
        for p in {G.SCENES[n].pipeline for n in G.names(gate)}:
            assert [n for n in G.names(gate, (p,)) if sides[n][0]] and [n for n in G.names(gate, (p,)) if not sides[n][0]], (gate, p)
    # X: the doubled trip, and the combination nobody had looked at: allowed with the culls off
    assert of("X", lambda s, cull, q, t, x2, r: x2 and cull) and of("X", lambda s, cull, q, t, x2, r: not x2 and cull)
    assert of("X", lambda s, cull, q, t, x2, r: x2 and not cull) and of("X", lambda s, cull, q, t, x2, r: not x2 and not cull)
    for label in ("cx", "cy", "cz", "md"):
        mine = [n for n in G.names("X") if f"/{label}" in n]
        assert {sides[n][3] for n in mine} == ({False} if label == "cz" else {True, False}), label
    # M: every round length and none, the quick cull on and off
    assert {sides[n][4] for n in G.names("M", ("julia_24",))} == {0, 16}
    assert {sides[n][4] for n in G.names("M", ("genjulia",))} == {0, 8, 16}
    assert {sides[n][4] for n in G.names("M", ("sphere",))} == {0, 8}
    assert of("M", lambda s, cull, q, t, x2, r: cull and not q and not s.heatmap) and of("M", lambda s, cull, q, t, x2, r: q)
    # O, H
    for gate, k in (("O", 0), ("H", 2)):
        for p in {G.SCENES[n].pipeline for n in G.names(gate)}:
            assert {sides[n][k] for n in G.names(gate, (p,))} == {True, False}, (gate, p)
    # the stated side agrees with the gate for the rows whose gate is one comparison
    for n in G.names("RDO"):
        s = G.SCENES[n]
        if s.side in ("below", "inside"):
            assert sides[n][0], n
        if s.side in ("at", "above"):
            assert not sides[n][0], n
    assert set(G.GATES) == {s.gate for s in G.SCENES.values()}


def test_the_caps_hold_and_the_launches_have_rounds_to_lose():
    for n, s in G.SCENES.items():
        assert G.caps_hold(s), n
        assert s.size == F.FRAME or s.gate in "HMS", n
    for L in G.plan("wave"):
        s = G.SCENES[L.scene]
        assert len(L.cams) == s.views and (s.lone or F.tiles(*L.size) * s.views >= F.REQUEUE_MIN_WORKGROUPS), L.label
    assert {G.SCENES[L.scene].gate for L in G.plan("block")} == set(G.CHILD_GATES)
    assert set(G.WAVE_GATES) <= set(G.CHILD_GATES)


def test_far_origin_images_are_on_their_side(kifs):
    for n in G.names("O"):
        for c in range(len(G.CAMERAS)):
            o = np.array(G.camera(kifs, n, c).into_buffer_data().origin[:], dtype=np.float64)
            assert (float((o * o).sum()) < 1.0e30) == (G.SCENES[n].side == "below"), (n, c)
    images = {bytes(kifs.uniform_bytes(G.camera(kifs, G.names("O")[0], c).into_buffer_data())) for c in range(4)}
    assert len(images) == 4


def test_neighbours_are_f32_neighbours():
    f = np.float32
    assert f(G.below(G.SANE_FAR)) < f(1.0e15) == f(G.SANE_FAR) < f(G.above(G.SANE_FAR))
    assert np.nextafter(f(G.below(G.X2_LO)), f(1)) == f(2.0 ** -14) and np.nextafter(f(G.above(G.X2_HI)), f(0)) == f(2.0 ** 10)
    assert np.nextafter(f(G.above(G.X2_FAR)), f(0)) == f(2.0 ** 60)
    assert f(1.0) + f(999998.0) == f(999999.0) and f(2.0) + f(999998.0) == f(1.0e6) and f(2.0) + f(999997.0) < f(1.0e6)


@pytest.mark.parametrize("gate", [g for g in G.GATES])
def test_cases_show_what_the_table_says(gate, oracle, kifs):
    """Non-vacuity: a `fractal` case has >= 1 % of some view off the background and >= 8 distinct colours, a
    `background_only` case does not (so the table cannot go stale in either direction)."""
    for n in G.names(gate):
        s = G.SCENES[n]
        share, colours = shown(oracle, kifs, n)
        print(f"{n}: {100 * share:.2f} % of a view, {colours} colours: {s.shows}")
        fractal = share >= MIN_SHARE and colours >= MIN_COLOURS
        assert fractal == (s.shows == "fractal"), (n, share, colours)


def test_at_most_a_third_is_background_and_every_gate_shows_the_fractal_on_each_side():
    cases = [s for s in G.SCENES.values()]
    assert 3 * sum(s.shows == "background_only" for s in cases) <= len(cases)
    assert {n for n, s in G.SCENES.items() if s.shows == "background_only"} == G.BACKGROUND_ONLY
    for gate, (on, off) in SIDES.items():
        for side in (on, off):
            if isinstance(side, str):
                continue  # empty by construction: the sentence in option_gates.py says why
            assert any(G.SCENES[n].shows == "fractal" for n in G.names(gate) if side(n)), (gate, side)


def _s(k, want=True):
    return lambda n: bool(G.gate_sides(G.SCENES[n])[k]) == want


# per gate: which cases are on either side of it (a string: that side is empty by construction)
SIDES = {
    "E": (lambda n: G.gate_sides(G.SCENES[n])[4] > 0 or G.gate_sides(G.SCENES[n])[0], "epsilon < 0 or NaN hits nothing"),
    "R": (_s(0), _s(0, False)),
    "D": (_s(0), _s(0, False)),
    "X": (_s(3), _s(3, False)),
    "M": (lambda n: G.gate_sides(G.SCENES[n])[4] > 0, lambda n: G.gate_sides(G.SCENES[n])[4] == 0),
    "H": (_s(2), _s(2, False)),
}


def test_expected_tuple_agrees_with_the_cpu_driver():
    """SHAPE_CASES of tests/hip_stub/host_driver.cpp, "steps:", "heatmap", "epsilon 0" and "lone Julia": the round
    lengths the host gives a launch without knobs; the `group2` configuration forces the shape and leaves them."""
    def rounds(name, config="group2"):
        L = next(L for L in G.plan(config) if L.scene == name)
        return G.expected_tuple(config, L)[3]

    assert rounds("M/julia_24/mi=32") == 16 and rounds("M/julia_24/mi=31") == 0
    assert rounds("M/sphere/mi=16") == 8 and rounds("M/sphere/mi=15") == 0
    assert rounds("M/sierpinski/mi=16") == 8 and rounds("M/sierpinski/mi=15") == 0
    assert [rounds(f"M/genjulia/mi={k}") for k in (32, 31, 16, 15)] == [16, 8, 8, 0]
    assert rounds("M/julia_24/mi=64/lone") == 32 and rounds("M/julia_24/mi=63/lone") == 16
    assert rounds("M/sphere/mi=16", "wave") == 4 and rounds("M/julia_24/mi=32", "wave") == 16
    for name in ("M/julia_24/mi=0", "M/julia_24/mi=-5", "M/julia_24/mi=0/heatmap", "E/julia_24/eps=0", "E/sphere/eps=nan",
                 "E/sierpinski/eps=-1e-3"):
        for config in G.CONFIGS:
            L = next(L for L in G.plan(config) if L.scene == name)
            assert G.expected_tuple(config, L) == ("render_kernel", -1, -1, 0), (name, config)
    for config in G.CONFIGS:  # the block form has no rounds anywhere; elsewhere fill_params' value stands for a batch
        for L in G.plan(config):
            s = G.SCENES[L.scene]
            want = G.gate_sides(s)[4]
            if config == "block":
                want = 0
            elif s.lone and want == 16 and s.max_iterations >= 64:
                want = 32
            elif config == "wave" and want == 8 and s.group == F.KIFS:
                want = 4
            assert G.expected_tuple(config, L)[3] == want, (config, L.label)


def test_the_light_shows_in_a_fractal_case_of_every_gate_pipeline(oracle, kifs):
    """The rows of test_lit_frame and test_occlusion_frame (tests/test_gpu_option_gates.py) cannot pass with the light
    or the term ignored: for each of the five gate pipelines some case shown as `fractal` has, at the size and from the
    cameras of those tests, lit bytes under light A and the default term that are not the oracle's plain bytes, and a
    factor below 1."""
    O, K = oracle, kifs
    size, cams = (64, 48), (1, 2)  # GEOMETRY and GEOMETRY_CAMERAS of tests/test_gpu_option_gates.py
    ub = K.uniform_bytes
    screen = O.from_bytes(O.Screen, ub(K.ScreenData(*size).into_buffer_data()))
    assert set(G.PIPELINES) == {G.SCENES[n].pipeline for n in G.names("ERDXIM")} and len(G.PIPELINES) == 5
    for p in G.PIPELINES:
        lit, occluded = [], []
        for n in G.names("ERDXIM", (p,)):
            if G.SCENES[n].shows != "fractal" or G.SCENES[n].heatmap:
                continue
            options, it = O.from_bytes(O.Options, ub(G.options(K, n))), O.iters(*G.SCENES[n].iters)
            for c in cams:
                camera = O.from_bytes(O.Camera, ub(G.camera(K, n, c).into_buffer_data()))
                m = LR.march(O, screen, camera, options, it, LR.A, OR.DEFAULT)
                if (LR.encode(O, m.rgb, 1) != O.render(screen, camera, options, it, encode=1)).any():
                    lit.append((n, c))
                if (m.hit & (m.a < 1)).any():
                    occluded.append((n, c))
        print(p, ": views whose lit bytes are not the plain frame's:", len(lit), "; views with a factor below 1:", len(occluded))
        assert lit and occluded, p
