"""tests/fold_trap_reference.c IS the contract of kifs_render_folded_trapped_async on the oracle.  With a neutral trap its
frame is tests/fold_reference.c's bit for bit (identity a); with no iterations of the fold it is tests/trap_reference.c's,
and so is its u (identity b), for every KIFS pipeline; the orbit gives its known answers, exact in f32; and the frames and
evaluation cases of tests/test_gpu_fold_trap.py do exercise the orbit: the named frames use both segments of the gradient
and differ from the folded and from the trapped unfolded frame, the least distance is attained at z_0, at a fold point and
at a base point often enough, and the stop rule cuts orbits.  That is what makes the GPU comparison mean something.
CPU only."""
import numpy as np
import pytest

import fold_reference as FR
import fold_trap_reference as FT
import lighting_reference as LR
import occlusion_reference as OR
import trap_reference as TR
from geometry_cases import cases
from helpers import oracle_uniforms
from test_fold_reference import KIFS_PIPELINES, UNFOLDED

GW, GH = 102, 45       # the frames of the GPU tests
f32 = np.float32
NEUTRAL = dict(FT.POINT8, scale=0.0, bias=0.0)


def _ext(oracle, on):
    return oracle.Ext(1, 64, 8.0, 0.02, 10.0) if on else None


def _uniforms(oracle, kifs, scene):
    screen, cam, gui, iters = scene
    s, c, o = oracle_uniforms(oracle, kifs, (screen, cam, gui))
    return s, c, o, oracle.iters(*iters)


def _heat(kifs, gui):
    return kifs.GuiData(**{**gui.__dict__, "is_heatmap": True, "fractal_color": (255, 128, 30)})


# ---- identity (a): a neutral trap gives the folded model's frame
@pytest.mark.parametrize("name", KIFS_PIPELINES)
def test_a_neutral_trap_is_the_folded_models_frame(name, kifs, oracle):
    s, c, o, it = _uniforms(oracle, kifs, cases(kifs, GW, GH)[name])
    want = FR.march(oracle, s, c, o, it, FR.ALL_STAGES, LR.A, OR.DEFAULT, None)
    fc = tuple(float(v) for v in o.fractal_color)
    for trap in (NEUTRAL, dict(FT.POINT8, mid=fc, far=fc)):
        got = FT.march(oracle, s, c, o, it, FR.ALL_STAGES, trap, LR.A, OR.DEFAULT, None)
        assert (got.hit == want.hit).all() and FT.same_bits(got.pos, want.pos).all()
        assert FT.same_bits(got.rgb, want.rgb).all(), name
        assert np.isinf(got.u[~got.hit]).all() and np.isfinite(got.u[got.hit]).all()


@pytest.mark.parametrize("name", ["box", "sierpinski"])
def test_a_neutral_trap_with_shadows_a_null_light_and_heatmap(name, kifs, oracle):
    screen, cam, gui, iters = cases(kifs, GW, GH)[name]
    s, c, o, it = _uniforms(oracle, kifs, (screen, cam, gui, iters))
    e = _ext(oracle, True)
    assert FT.same_bits(FT.march(oracle, s, c, o, it, FR.ALL_STAGES, NEUTRAL, LR.A, OR.DEFAULT, e).rgb,
                        FR.march(oracle, s, c, o, it, FR.ALL_STAGES, LR.A, OR.DEFAULT, e).rgb).all()
    assert FT.same_bits(FT.march(oracle, s, c, o, it, FR.ALL_STAGES, NEUTRAL, None, None, e).rgb,
                        FR.march(oracle, s, c, o, it, FR.ALL_STAGES, None, None, e).rgb).all()
    s, c, o, it = _uniforms(oracle, kifs, (screen, cam, _heat(kifs, gui), iters))
    heat = FT.march(oracle, s, c, o, it, FR.ALL_STAGES, FT.POINT8, LR.A, OR.DEFAULT, e)  # (any trap: the colour is the counter's)
    assert FT.same_bits(heat.rgb, FR.march(oracle, s, c, o, it, FR.ALL_STAGES, LR.A, OR.DEFAULT, e).rgb).all()
    assert np.isfinite(heat.u[heat.hit]).all() and heat.hit.any()  # ... and the plane still holds every hit's u


# ---- identity (b): no iterations of the fold give the trapped model's frame and u
@pytest.mark.parametrize("name", KIFS_PIPELINES)
def test_no_iterations_is_the_trapped_models_frame(name, kifs, oracle):
    s, c, o, it = _uniforms(oracle, kifs, cases(kifs, GW, GH)[name])
    for light, ao, shadows in ((LR.A, OR.DEFAULT, False), (None, None, True)):
        want = TR.march(oracle, s, c, o, it, TR.S, light, ao, _ext(oracle, shadows))
        got = FT.march(oracle, s, c, o, it, UNFOLDED, TR.S, light, ao, _ext(oracle, shadows))
        assert (got.hit == want.hit).all() and FT.same_bits(got.pos, want.pos).all()
        assert FT.same_bits(got.rgb, want.rgb).all(), name
        assert FT.same_bits(got.u[got.hit], want.u[want.hit]).all()
    rng = np.random.default_rng(0xf01d7)
    pts = rng.uniform(-2.0, 2.0, (512, 3)).astype(f32)
    for K in (0, 1, 6, 32):
        trap = dict(TR.S, iterations=K)
        assert FT.same_bits(FT.eval_u(oracle, o, UNFOLDED, trap, pts), TR.eval_u(oracle, o, trap, pts)).all(), (name, K)


# ---- the orbit's known answers, exact in f32
def test_known_answers(kifs, oracle):
    screen, cam, gui, iters = cases(kifs, GW, GH)["sphere"]
    _, _, o = oracle_uniforms(oracle, kifs, (screen, cam, gui))
    origin = dict(centre=(0.0, 0.0, 0.0, 0.0), axes=15)
    # ABS, N = 1, s = 2, c = (3, 0, 0): (1.5, 0, 0) folds onto the origin -- 2 * 1.5 - 3 = 0
    for K, want in ((0, 1.5), (1, 0.0), (8, 0.0)):
        u, info = FT.eval_u(oracle, o, FR.WIDE, dict(origin, iterations=K), [(1.5, 0.0, 0.0), (-1.5, 0.0, 0.0)], info=True)
        assert (u == f32(want)).all(), (K, u)
        assert (info[:, 0] == (1 if K else 0)).all() and (info[:, 1] == 0).all()
    # a position at or beyond max_distance has no fold point: u = d(z_0)
    _, _, near = oracle_uniforms(oracle, kifs, (screen, cam, kifs.GuiData(**{**gui.__dict__, "max_distance": 10.0})))
    u, info = FT.eval_u(oracle, near, FR.WIDE, dict(origin, iterations=8), [(20.0, 0.0, 0.0)], info=True)
    assert u[0] == f32(20.0) and tuple(info[0]) == (0, 1, 0)
    # ... where the same position within max_distance folds to (2 * 20 - 3, 0, 0), farther from the trap
    u, info = FT.eval_u(oracle, o, FR.WIDE, dict(origin, iterations=8), [(20.0, 0.0, 0.0)], info=True)
    assert u[0] == f32(20.0) and tuple(info[0]) == (0, 0, 1)
    u = FT.eval_u(oracle, o, FR.WIDE, dict(centre=(37.0, 0.0, 0.0, 0.0), axes=15, iterations=8), [(20.0, 0.0, 0.0)])
    assert u[0] == f32(0.0)
    # K < N drops the later fold points.  s = 2, c = (1, 0, 0), no stage: x -> 2 x - 1, so 0.75 -> 0.5 -> 0 -> -1; a plane
    # trap at x = 0 sees the zero at fold point 2
    line = dict(stages=0, iterations=3, scale=2.0, offset=(1.0, 0.0, 0.0))
    plane = dict(centre=(0.0, 0.0, 0.0, 0.0), axes=1)
    for K, want in ((0, 0.75), (1, 0.5), (2, 0.0), (3, 0.0)):
        assert FT.eval_u(oracle, o, line, dict(plane, iterations=K), [(0.75, 5.0, -7.0)])[0] == f32(want), K
    # Sierpinski base, N = 1, K = 3: one fold point and two base points.  s = 1 folds nothing: the fold point is p, and
    # the base points are the trapped call's first two from p
    _, _, sier = oracle_uniforms(oracle, kifs, cases(kifs, GW, GH)["sierpinski"][:3])
    still = dict(stages=0, iterations=1, scale=1.0, offset=(0.0, 0.0, 0.0))
    p = np.random.default_rng(0x51e2).uniform(-1.0, 1.0, (64, 3)).astype(f32)
    corner = dict(centre=(1.0, 1.0, 1.0, 0.0), axes=7)
    got, info = FT.eval_u(oracle, sier, still, dict(corner, iterations=3), p, info=True)
    assert FT.same_bits(got, TR.eval_u(oracle, sier, dict(corner, iterations=2, scale=0.0, bias=0.0, mid=TR.MID, far=TR.FAR), p)).all()
    assert (got != TR.eval_u(oracle, sier, dict(corner, iterations=1, scale=0.0, bias=0.0, mid=TR.MID, far=TR.FAR), p)).any()  # the second base point counts
    assert (got != TR.eval_u(oracle, sier, dict(corner, iterations=3, scale=0.0, bias=0.0, mid=TR.MID, far=TR.FAR), p)).any()  # and there is no third
    assert (info[:, 0] == 2).any() and (info[:, 2] == 1).all()
    # ... and on the sphere the same orbit ends with its fold point
    assert FT.same_bits(FT.eval_u(oracle, o, still, dict(corner, iterations=3), p),
                        TR.eval_u(oracle, o, dict(corner, iterations=0, scale=0.0, bias=0.0, mid=TR.MID, far=TR.FAR), p)).all()
    # the gradient is the trapped model's
    for uu in (0.0, 0.3, 0.75, 1.5, float("inf"), float("nan")):
        import ctypes as C
        col = (C.c_float * 3)()
        t = FT.library(oracle).kft_colour(C.byref(o), C.byref(TR.trap(TR.S)), float(uu), col)
        tt, want = TR.colour(oracle, o, TR.S, uu)
        assert f32(t) == tt and FT.same_bits(np.array(list(col), dtype=f32), want).all(), uu


# ---- guards: the GPU tests' named frames
@pytest.mark.parametrize("name", list(FT.NAMED))
def test_the_named_frames_use_the_gradient_and_differ_from_both_parents(name, kifs, oracle):
    scene, fold, trap = FT.named_scene(oracle, kifs, cases, name, GW, GH)
    screen, cam, gui, iters = scene
    e = _ext(oracle, True)
    f = FT.frame(oracle, kifs, screen, cam, gui, iters, fold, trap, LR.A, OR.DEFAULT, e)
    folded = FR.folded_frame(oracle, kifs, screen, cam, gui, iters, fold, LR.A, OR.DEFAULT, e)
    trapped = TR.trapped_frame(oracle, kifs, screen, cam, gui, iters, trap, LR.A, OR.DEFAULT, e)
    s, b = f32(trap["scale"]), f32(trap["bias"])
    t = np.clip(s * f.u[f.hit] + b, 0.0, 1.0)
    lower, upper = int(((t > 0) & (t < 0.5)).sum()), int(((t >= 0.5) & (t < 1)).sum())
    from_folded = int((FT.encode(oracle, f.rgb, 1) != FR.encode(oracle, folded.rgb, 1)).any(-1).sum())
    from_trapped = int((FT.encode(oracle, f.rgb, 1) != TR.encode(oracle, trapped.rgb, 1)).any(-1).sum())
    print(name, "hits", int(f.hit.sum()), "range", trap["scale"], trap["bias"], "lower segment", lower, "upper segment", upper,
          "differs from the folded frame in", from_folded, "and from the trapped unfolded frame in", from_trapped)
    assert f.hit.sum() >= 100 and (f.hit == folded.hit).all()
    assert lower >= 20 and upper >= 20
    assert from_folded >= 50 and from_trapped >= 50


@pytest.mark.parametrize("name", KIFS_PIPELINES)
def test_the_point_trap_recolours_every_pipeline(name, kifs, oracle):
    s, c, o, it = _uniforms(oracle, kifs, cases(kifs, GW, GH)[name])
    f = FT.march(oracle, s, c, o, it, FR.ALL_STAGES, FT.POINT8, LR.A)
    folded = FR.march(oracle, s, c, o, it, FR.ALL_STAGES, LR.A)
    recoloured = int((FT.encode(oracle, f.rgb, 1) != FR.encode(oracle, folded.rgb, 1)).any(-1).sum())
    print(name, "hits", int(f.hit.sum()), "recoloured", recoloured)
    if name != "unknown_id":  # (the constant 1 is never hit)
        assert recoloured >= 50


# ---- guards: the evaluation cases
def test_the_evaluation_cases_reach_every_part_of_the_orbit(kifs, oracle):
    total = {}
    for name in FT.EVAL_PIPELINES:
        _, _, o = oracle_uniforms(oracle, kifs, FT.eval_scene(kifs, cases, name)[:3])
        assert o.max_distance == f32(FT.EVAL_MAX_DISTANCE)
        pts = FT.eval_points(name)
        assert (np.linalg.norm(pts.astype(np.float64), axis=1) < 2.5).all()
        n = at0 = at_fold = at_base = cut = 0
        for fold, trap in FT.eval_cases():
            _, info = FT.eval_u(oracle, o, fold, trap, pts, info=True)
            n += len(pts)
            at0 += int((info[:, 0] == 0).sum())
            at_fold += int((info[:, 0] == 1).sum())
            at_base += int((info[:, 0] == 2).sum())
            cut += int(info[:, 1].sum())
        total[name] = (n, at0, at_fold, at_base, cut)
        print(name, "cases", n, "least distance at z_0", at0 / n, "at a fold point", at_fold / n, "at a base point", at_base / n,
              "orbits cut by the stop rule", cut / n)
        assert at0 >= 0.05 * n and at_fold >= 0.05 * n and cut >= 0.01 * n, name
        assert (at_base >= 0.05 * n) if name == "sierpinski" else at_base == 0, name
