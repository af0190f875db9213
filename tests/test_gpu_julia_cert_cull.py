"""The certified cull radius of the power-2 Julia set on the GPU, byte for byte: every frame a launch writes with the cull's
thresholds on the certified radius equals the CPU oracle's frame -- the oracle marches every ray and knows no cull -- AND
the frame of the same build with KIFS_JULIA_CERT_CULL=0 (the patch sphere's thresholds).  Scenes, views and launches:
tests/julia_cert_cull_cases.py; one child process per kernel form and switch position (the knobs are read once per
process): render_kernel, render_group_kernel with one and two tiles, render_wave_kernel.  The render_kernel children also
run the other entry points: a batch of 3, a band, supersampling, the geometry output, adaptive anti-aliasing, animated
launches whose frames bring their own constants, accumulated frames.

Non-vacuity (no measurement: NumPy on the rays' closest approaches): for every view at distance >= 2.05 of a scene with a
certificate the new cull takes at least 25 % of the rays today's cull marches.
"""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import julia_cert_cull_cases as X
from helpers import oracle_frame

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
_ORACLE = {}


def _radius(scene):
    from kifs_raymarching_amd._lib import lib
    c, sdf_iters, eps, _ = X.SCENES[scene]
    return lib.kifs_host_julia_cull_radius((C.c_float * 4)(*c), eps, 1000.0, sdf_iters, None)


def _frame(oracle, kifs, scene, view_index):
    key = (scene, view_index)
    if key not in _ORACLE:
        w, h = X.SCENES[scene][3]
        _ORACLE[key] = oracle_frame(oracle, kifs, kifs.ScreenData(w, h), X.view(kifs, view_index), X.options(kifs, scene),
                                    X.iters(scene))
    return _ORACLE[key]


def _closest_approach2(kifs, scene, view_index):
    """(H, W) squared closest approach of every pixel's ray to the origin as ray_never_inside defines it (|origin|^2 for
    a ray that points away), in double."""
    w, h = X.SCENES[scene][3]
    u = X.view(kifs, view_index).u
    org = np.array([u.origin[k] for k in range(3)], dtype=np.float64)
    m = np.array([[u.matrix[c][r] for r in range(3)] for c in range(3)], dtype=np.float64)
    ys, xs = np.mgrid[0:h, 0:w]
    ux = 2.0 * (xs + 0.5) / h - float(F(w) / F(h))
    uy = 2.0 * (ys + 0.5) / h - 1.0
    d = np.stack([ux * m[1][k] - uy * m[2][k] - m[0][k] for k in range(3)], axis=-1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    b = -(d @ org)
    return np.where(b <= 0.0, org @ org, org @ org - b * b)


def test_the_certificates_of_the_scenes(kifs):
    for scene in X.SCENES:
        rho = _radius(scene)
        assert (rho == 0.0) == scene.startswith("nocert"), scene
    radii = {c: _radius(s) for s, c in (("headline_256", "h"), ("reference_96", "r"), ("small_256", "s"))}
    assert radii["s"] < radii["h"] < radii["r"] < 2.0


@pytest.mark.parametrize("scene", [s for s in X.SCENES if not s.startswith("nocert")])
def test_the_new_cull_is_not_vacuous(kifs, scene):
    rho, eps = _radius(scene), X.SCENES[scene][2]
    R = F(2.0) + F(eps)
    today = float(F(1.1) * R * R)
    new = float((F(1.0) + F(2.0 ** -6)) * F(rho) * F(rho))
    for v, (distance, _, _, _) in enumerate(X.VIEWS):
        if distance < 2.05:
            continue
        c2 = _closest_approach2(kifs, scene, v)
        marched = c2 <= today
        share = float((marched & (c2 > new)).sum()) / float(marched.sum())
        print(f"{scene} view {v} (distance {distance}): {int(marched.sum())} rays marched today, {share:.3f} of them culled")
        assert share >= 0.25, (scene, v, share)


def _run_child(tmp_path_factory, form, switch_on, extras):
    out = tmp_path_factory.mktemp("cert_cull") / f"{form}_{int(switch_on)}.npz"
    cmd = [sys.executable, str(ROOT / "tests" / "julia_cert_cull_child.py"), str(out)] + (["extras"] if extras else [])
    p = subprocess.run(cmd, env=X.child_env(os.environ, form, switch_on), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    cache = {}

    def get(form, switch_on):
        if (form, switch_on) not in cache:
            cache[form, switch_on] = _run_child(tmp_path_factory, form, switch_on, extras=form == "block")
        return cache[form, switch_on]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(X.FORMS))
def test_every_form_equals_the_oracle_and_the_switched_off_build(kifs, oracle, children, form):
    on, off = children(form, True), children(form, False)
    kernel, group_tiles = X.FORMS[form][1]
    for i, (scene, views) in enumerate(X.launches()):
        for run in (on, off):
            assert str(run[f"L{i}_kernel"][0]) == kernel and int(run[f"L{i}_shape"][0]) == group_tiles, (scene, run[f"L{i}_kernel"])
            assert int(run[f"L{i}_shape"][1]) == (0 if form == "block" else 16)
            assert bool(run[f"L{i}_copies_equal"][0]), (form, scene)
        distinct = [int(v) for v in on[f"L{i}_views"]]
        assert distinct == sorted(set(views)) == [int(v) for v in off[f"L{i}_views"]]
        for k, v in enumerate(distinct):
            want = _frame(oracle, kifs, scene, v)
            got, plain = on[f"L{i}_frames"][k], off[f"L{i}_frames"][k]
            assert np.array_equal(got, want), (form, scene, v, int((got != want).any(-1).sum()))
            assert np.array_equal(plain, want), (form, scene, v, int((plain != want).any(-1).sum()))
            assert X.digest(got) == X.digest(plain)


@pytest.mark.gpu
def test_the_other_entry_points(kifs, oracle, children):
    import aa_reference as AA
    import accumulate_reference as ACC
    import adaptive_reference as AD
    import geometry_reference as GR
    on, off = children("block", True), children("block", False)
    scene = X.EXTRA_SCENE
    w, h = X.SCENES[scene][3]
    screen, gui, it = kifs.ScreenData(w, h), X.options(kifs, scene), X.iters(scene)
    cam5, cam2 = X.view(kifs, 0), X.view(kifs, 1)
    for key in on:
        if not key.startswith("L"):
            assert on[key].shape == off[key].shape and X.digest(on[key]) == X.digest(off[key]), key
    # a batch of 3 poses
    for k in range(3):
        assert np.array_equal(on["batch3"][k], _frame(oracle, kifs, scene, k)), k
    # a band
    y0, y1 = X.BAND
    assert np.array_equal(on["band"], _frame(oracle, kifs, scene, 1)[y0:y1])
    # supersampling
    assert np.array_equal(on["ssaa2"], AA.aa_frame(oracle, kifs, screen, cam5, gui, it, 2))
    # the geometry output: the oracle's march; t = +inf and a zero normal on every pixel the new cull removes
    rho = _radius(scene)
    new = float((F(1.0) + F(2.0 ** -6)) * F(rho) * F(rho))
    for k, (cam, v) in enumerate(((cam5, 0), (cam2, 1))):
        geom, hit, _ = GR.geometry_frame(oracle, kifs, screen, cam, gui, it)
        assert GR.same_bits(on["geometry"][k], geom).all()
        assert np.array_equal(on["geometry_colour"][k], _frame(oracle, kifs, scene, v))
        culled = _closest_approach2(kifs, scene, v) > new * 1.001
        assert culled.sum() > 1000 and not hit[culled].any()
        assert np.isposinf(on["geometry"][k][culled][:, 3]).all() and (on["geometry"][k][culled][:, :3] == 0.0).all()
        # adaptive anti-aliasing
        want, mask = AD.expected_frame(oracle, kifs, screen, cam, gui, it, 2, 0.9, 0.05, geom=geom)
        assert np.array_equal(on["adaptive"][k], want) and int(on["adaptive_counts"][k]) == int(mask.sum())
    # animated launches: every frame is the oracle's for its own constant
    for a, constants in enumerate(X.ANIMATIONS):
        for k, (c, cam) in enumerate(zip(constants, (cam5, cam2))):
            want = oracle_frame(oracle, kifs, screen, cam, X.options(kifs, scene, c), it)
            assert np.array_equal(on[f"animation{a}"][k], want), (a, k)
    # accumulated frames
    sub = [kifs.CameraData(origin_distance=d, min_distance=0.05, phi=p, theta=t) for d, p, t in X.ACCUMULATE_VIEWS]
    assert np.array_equal(on["accumulate"], ACC.accumulate_frames(oracle, kifs, screen, sub, gui, it, 4))
    opts = [X.options(kifs, scene, c) for c in (X.HEADLINE_C, X.SMALL_C, X.HEADLINE_C, X.REFERENCE_C)]
    assert np.array_equal(on["accumulate_options"], ACC.accumulate_frames(oracle, kifs, screen, sub, opts, it, 4))
