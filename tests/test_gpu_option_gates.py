"""The kernels against the oracle on both sides of every option gate of kifs_schedule.cpp (tests/option_gates.py has the
table, tests/test_option_gates_plan.py says on the CPU which side each case is on and what it shows, GATE_CASES of
tests/hip_stub/host_driver.cpp pins the host's decisions).  Everything is compared bit for bit with the oracle on the
product's own uniform bytes; there is no tolerance.  Destinations are pre-filled with a sentinel no encode produces.

  forms      the block, group1, group2 and wave forms, one child process each with the KIFS_TUNING knobs of
             kernel_forms.CONFIGS (tests/kernel_forms_child.py, given this table): every case of E, R, D, X, M, I, P, O and
             H as a batch, the M 63 / 64 pair as lone frames; the debug tuple, identical views per camera, the oracle's bytes
  lone       the S screens and every E, D and M case at 96 x 64 through GraphicState.render, both encodes
  geometry   E, R, D, X and I at 64 x 48: render_geometry's texels against tests/geometry_reference.py -- the f32 t and normal
             show a wrong square root or orbit trip that a colour byte may round away
  rays       1024 generated rays in every E, D, X, M (0, -5) and P scene against tests/ray_reference.py, texels and bytes
  shading    E, R, D, X, I and M at 64 x 48 through kifs_render_lit_async (light A, the default term) and
             kifs_render_occlusion_async (the default term, with its plane) against tests/lighting_reference.py and
             tests/occlusion_reference.py: both kernels take the culls, the doubled trip and the rounds' permissions from the
             same launch parameters as the plain forms and shade from a second reading of them

Children run one after another, each under `timeout`.  A child that ends with any other status than 0 stops the module,
as in tests/test_gpu_kernel_forms.py: every later parameter of the forms fails without starting anything."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import geometry_reference as GR
import kernel_forms as F
import lighting_reference as LR
import occlusion_reference as OR
import option_gates as G
import ray_cases
import ray_reference as RR
from geometry_cases import Raw
from helpers import diff_report

pytestmark = pytest.mark.gpu

CHILD = Path(__file__).resolve().parent / "kernel_forms_child.py"
ROOT = CHILD.parent.parent
SENT_U8 = 0x5A
SENT_F32 = np.float32(-12345.5)
LONE = (96, 64)
GEOMETRY = (64, 48)
GEOMETRY_CAMERAS = (1, 2)   # on the bounding sphere, just outside the quick-exit sphere
RAY_SEED, RAYS = 5, 1024

_RESULTS = {}   # config -> (launches checked, failures)
_STOPPED = []   # [(config, status)] once a child has not ended cleanly
_ORACLE = {}    # (scene, camera, encode, size) -> frame, shared by every test of the session


def _uniforms(O, K, name, size, cam):
    ub = K.uniform_bytes
    return (O.from_bytes(O.Screen, ub(K.ScreenData(*size).into_buffer_data())),
            O.from_bytes(O.Camera, ub(G.camera(K, name, cam).into_buffer_data())),
            O.from_bytes(O.Options, ub(G.options(K, name))))


def _oracle(O, K, name, cam, encode, size):
    key = (name, cam, encode, size)
    if key not in _ORACLE:
        s, c, o = _uniforms(O, K, name, size, cam)
        frame = O.render(s, c, o, O.iters(*G.SCENES[name].iters), encode=encode)
        frame.setflags(write=False)
        _ORACLE[key] = frame
    return _ORACLE[key]


# ---- forms ------------------------------------------------------------------------------------------------------------
def _child(config, tmp):
    out = tmp / f"{config}.npz"
    limit = G.CONFIGS[config].timeout
    try:
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, str(CHILD), config, str(out), "option_gates"],
                           cwd=str(ROOT), env=F.child_env(os.environ, config), capture_output=True, text=True,
                           timeout=limit + 60)
    except subprocess.TimeoutExpired as e:  # (`timeout` itself did not end it: counts as its time limit)
        return 124, str(e.stdout or "")[-3000:], out
    return p.returncode, (p.stdout + p.stderr)[-3000:], out


def _check(config, data, O, K):
    """(labels checked, failures) of one configuration's output."""
    checked, failures = set(), []
    for i, L in enumerate(G.plan(config)):
        want_tuple = G.expected_tuple(config, L)
        got = [(str(k), int(a), int(b), int(c)) for k, (a, b, c) in zip(data[f"L{i}_kernels"], data[f"L{i}_shape"])]
        if any(g != want_tuple for g in got):
            failures.append((L.label, "debug tuple", got, want_tuple))
            continue
        digests = data[f"L{i}_digests"]
        first = {c: v for v, c in reversed(list(enumerate(L.cams)))}
        if not all(digests[r, v] == digests[0, first[c]] for r in range(L.repeats) for v, c in enumerate(L.cams)):
            failures.append((L.label, "views of one camera differ"))
            continue
        bad = []
        for cam, view in zip(data[f"L{i}_cams"], data[f"L{i}_views"]):
            if (view[..., 3] == SENT_U8).any():
                bad.append((int(cam), "pixels never written"))
                continue
            rep = diff_report(view, _oracle(O, K, L.scene, int(cam), L.encode, L.size))
            if rep["mismatched_pixels"] != 0:
                bad.append((int(cam), rep))
        if bad:
            failures.append((L.label, "pixels differ from the oracle", want_tuple, bad))
            continue
        checked.add(L.label)
    return checked, failures


def _verified(config, tmp_path_factory, O, K):
    if config not in _RESULTS:
        if _STOPPED:
            pytest.fail(f"not started: {_STOPPED[0][0]} ended with {_STOPPED[0][1]}")
        rc, tail, out = _child(config, tmp_path_factory.mktemp("gates"))
        if rc != 0:
            _STOPPED.append((config, rc))
            _RESULTS[config] = (set(), [f"the child ended with {rc}:\n{tail}"])
        else:
            with np.load(out) as data:
                _RESULTS[config] = _check(config, data, O, K)
            out.unlink()
    return _RESULTS[config]


@pytest.mark.parametrize("config", list(G.CONFIGS))
def test_form(config, tmp_path_factory, oracle, kifs):
    """Every gate case in one forced form: the debug tuple it must report, identical views per camera, the oracle's
    bytes.  Every gate has a case on each side in every form (the wave form matters for E, R, D, X, O and H)."""
    checked, failures = _verified(config, tmp_path_factory, oracle, kifs)
    assert not failures, failures
    assert checked == {L.label for L in G.plan(config)}
    assert {G.SCENES[n].gate for n in checked} == set(G.CHILD_GATES)


# ---- lone frames ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ogs(kifs):
    g = kifs.GraphicState(0)
    yield g
    g.close()


def _scene(g, K, name, size):
    g.update_screen_data(K.ScreenData(*size))
    g.set_raw_uniforms(options=G.options(K, name))
    g.set_iters(*G.SCENES[name].iters)
    g.set_extensions(soft_shadow=False)
    g.set_supersampling(1)


def _lone(g, K, name, size, cam, encode):
    import torch
    w, h = size
    out = torch.full((h, w, 4), SENT_U8, dtype=torch.uint8, device="cuda:0")
    g.set_camera(G.camera(K, name, cam))
    g.render(out=out, encode=encode)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _assert_frame(got, want, what):
    assert not (got[..., 3] == SENT_U8).any(), f"{what}: pixels never written"
    rep = diff_report(got, want)
    assert rep["mismatched_pixels"] == 0, (what, rep)


@pytest.mark.parametrize("name", G.names("EDM"))
def test_lone_frame(name, ogs, kifs, oracle):
    _scene(ogs, kifs, name, LONE)
    for encode in (1, 0):
        for cam in (0, 2):
            _assert_frame(_lone(ogs, kifs, name, LONE, cam, encode), _oracle(oracle, kifs, name, cam, encode, LONE),
                          (name, cam, encode))


@pytest.mark.parametrize("name", G.names("S"))
def test_screen(name, ogs, kifs, oracle):
    """A screen of a few pixels, lone and as a 3-view batch, both encodes."""
    import torch
    size = G.SCENES[name].size
    w, h = size
    _scene(ogs, kifs, name, size)
    cams = (0, 2, 3)
    for encode in (1, 0):
        _assert_frame(_lone(ogs, kifs, name, size, 0, encode), _oracle(oracle, kifs, name, 0, encode, size), (name, "lone", encode))
        outs = torch.full((len(cams), h, w, 4), SENT_U8, dtype=torch.uint8, device="cuda:0")
        stream = torch.cuda.Stream()
        ogs.render_batch_async([outs[v] for v in range(len(cams))], [G.camera(kifs, name, c) for c in cams], stream=stream,
                               encode=encode)
        stream.synchronize()
        torch.cuda.synchronize()
        host = outs.cpu().numpy()
        for v, c in enumerate(cams):
            _assert_frame(host[v], _oracle(oracle, kifs, name, c, encode, size), (name, "batch", c, encode))


# ---- geometry planes --------------------------------------------------------------------------------------------------
def _assert_same_bits(got, want, what):
    same = GR.same_bits(got, want)
    if not same.all():
        at = tuple(np.argwhere(~same)[0])
        pytest.fail(f"{what}: {int((~same).sum())} of {same.size} floats differ; first at {at}: "
                    f"got {got[at]!r} ({got[at].view(np.uint32):#x}), want {want[at]!r} ({want[at].view(np.uint32):#x})")


@pytest.mark.parametrize("name", G.names("ERDXI"))
def test_geometry_plane(name, ogs, kifs, oracle):
    """Both cameras in one call on sentinel-filled planes: every texel (n.x, n.y, n.z, t) and every colour byte."""
    from test_gpu_geometry import _call, _texels
    w, h = GEOMETRY
    _scene(ogs, kifs, name, GEOMETRY)
    cams = [G.camera(kifs, name, c) for c in GEOMETRY_CAMERAS]
    ogs.set_camera(cams[0])
    st, colour, geom, _ = _call(ogs, kifs, cams=cams, count=len(cams))
    assert st == 0
    for v, c in enumerate(GEOMETRY_CAMERAS):
        s, cam, o = _uniforms(oracle, kifs, name, GEOMETRY, c)
        want, _, _ = GR.march(oracle, s, cam, o, oracle.iters(*G.SCENES[name].iters))
        texels = _texels(geom[v], w)
        assert not (texels == SENT_F32).any(), (name, c, "texels never written")
        _assert_same_bits(texels, want, (name, c))
        rep = diff_report(colour[v], _oracle(oracle, kifs, name, c, 1, GEOMETRY))
        assert rep["mismatched_pixels"] == 0, (name, c, rep)


# ---- ray queries ------------------------------------------------------------------------------------------------------
RAY_SCENES = [n for n in G.names("EDXMP") if G.SCENES[n].gate != "M" or G.SCENES[n].max_iterations <= 0]


@pytest.mark.parametrize("name", RAY_SCENES)
def test_ray_queries(name, ogs, kifs, oracle):
    from test_gpu_rays import _assert_bytes, _trace
    _scene(ogs, kifs, name, LONE)
    rays, _ = ray_cases.rays(RAY_SEED, RAYS)
    for encode in (1, 0):
        want_geom, want_rgba, _ = RR.trace_scene(oracle, kifs, Raw(G.options(kifs, name)), G.SCENES[name].iters, rays, encode)
        st, geom, rgba = _trace(ogs._ctx, rays, encode)
        assert st == 0
        _assert_same_bits(geom, want_geom, (name, encode))
        _assert_bytes(rgba, want_rgba, f"{name} encode={encode}")


# ---- the lit and the occlusion kernels ---------------------------------------------------------------------------------
SHADING_GATES = "ERDXIM"


def _shading_views(ogs, kifs, oracle, name):
    """The context set up for the case at the geometry planes' size, its two cameras, and per camera the oracle-side
    uniforms the models march with.  Cases the plan marks `background_only` are compared like the others."""
    _scene(ogs, kifs, name, GEOMETRY)
    cams = [G.camera(kifs, name, c) for c in GEOMETRY_CAMERAS]
    ogs.set_camera(cams[0])
    return cams, [_uniforms(oracle, kifs, name, GEOMETRY, c) for c in GEOMETRY_CAMERAS]


@pytest.mark.parametrize("name", G.names(SHADING_GATES))
def test_lit_frame(name, ogs, kifs, oracle):
    """Both cameras in one call of kifs_render_lit_async under light A with the default term: every colour byte."""
    from test_gpu_lighting import _assert_bytes, _call
    cams, uniforms = _shading_views(ogs, kifs, oracle, name)
    r = _call(ogs, kifs, LR.A, ao=OR.DEFAULT, cams=cams, count=len(cams))
    assert r.st == 0
    for v, (c, (s, cam, o)) in enumerate(zip(GEOMETRY_CAMERAS, uniforms)):
        m = LR.march(oracle, s, cam, o, oracle.iters(*G.SCENES[name].iters), LR.A, OR.DEFAULT)
        _assert_bytes(r.colour[v], LR.encode(oracle, m.rgb, 1), (name, c))


@pytest.mark.parametrize("name", G.names(SHADING_GATES))
def test_occlusion_frame(name, ogs, kifs, oracle):
    """Both cameras in one call of kifs_render_occlusion_async with the default term: every colour byte, and every
    factor of the plane by bit pattern."""
    from test_gpu_occlusion import _assert_bytes, _assert_plane, _call
    cams, uniforms = _shading_views(ogs, kifs, oracle, name)
    r = _call(ogs, kifs, OR.DEFAULT, cams=cams, count=len(cams))
    assert r.st == 0
    for v, (c, (s, cam, o)) in enumerate(zip(GEOMETRY_CAMERAS, uniforms)):
        m = OR.march(oracle, s, cam, o, oracle.iters(*G.SCENES[name].iters), OR.DEFAULT)
        _assert_bytes(r.colour[v], OR.encode(oracle, m.rgb, 1), (name, c))
        _assert_plane(r.plane[v], m.plane, (name, c))
