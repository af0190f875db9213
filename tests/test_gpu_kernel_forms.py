"""Every render kernel instantiation against the oracle, reached on purpose: each configuration of the form table
(tests/kernel_forms.py) forces one launch shape through the KIFS_TUNING knobs in a child process of its own
(tests/kernel_forms_child.py) and renders every scene of the configuration on the same ragged frame, bands, a batch
through the device view table, a shuffled tile order and lone frames.  This process never opens the GPU: it checks
the debug tuple every launch reports, that views of one camera are byte-identical and that every view equals the
oracle.  test_instantiation then names, per instantiation of the table, the configuration that checked it.

Children run one after another, each under `timeout`.  A child that ends with any other status than 0 -- a time limit
(124, 137), an abort (134), a segmentation fault (139), a signal or an exception -- stops the module: every later
parameter fails without starting anything."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import kernel_forms as F
from helpers import diff_report

pytestmark = pytest.mark.gpu

CHILD = Path(__file__).resolve().parent / "kernel_forms_child.py"
ROOT = CHILD.parent.parent

_RESULTS = {}   # config -> (names checked, failures)
_STOPPED = []   # [(config, status)] once a child has not ended cleanly
_ORACLE = {}    # (scene, camera, encode, size) -> frame: shared by every configuration of the session
_SHOWN = {}     # scene -> [background seen, fractal seen]


def _oracle(O, K, scene, cam, encode, size):
    key = (scene, cam, encode, size)
    if key not in _ORACLE:
        s, ub = F.SCENES[scene], K.uniform_bytes
        ext = F.extensions(scene)
        _ORACLE[key] = O.render(O.from_bytes(O.Screen, ub(K.ScreenData(*size).into_buffer_data())),
                                O.from_bytes(O.Camera, ub(F.camera(K, scene, cam).into_buffer_data())),
                                O.from_bytes(O.Options, ub(F.options(K, scene))), O.iters(*s.iters), encode=encode,
                                ext=O.Ext(1, ext["shadow_steps"], ext["shadow_k"], ext["shadow_t0"], ext["shadow_max_t"])
                                if s.shadow else None)
    return _ORACLE[key]


def _child(config, tmp):
    out = tmp / f"{config}.npz"
    limit = F.CONFIGS[config].timeout
    try:
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, str(CHILD), config, str(out)],
                           cwd=str(ROOT), env=F.child_env(os.environ, config), capture_output=True, text=True,
                           timeout=limit + 60)
    except subprocess.TimeoutExpired as e:  # (`timeout` itself did not end it: counts as its time limit)
        return 124, str(e.stdout or "")[-3000:], out
    return p.returncode, (p.stdout + p.stderr)[-3000:], out


def _check(config, data, O, K):
    """(instantiations checked, failures) of one configuration's output."""
    checked, failures = set(), []
    for i, L in enumerate(F.plan(config)):
        want_tuple = F.expected_tuple(config, L)
        got = [(str(k), int(a), int(b), int(c)) for k, (a, b, c) in zip(data[f"L{i}_kernels"], data[f"L{i}_shape"])]
        if any(g != want_tuple for g in got):
            failures.append((L.label, "debug tuple", got, want_tuple))
            continue
        digests = data[f"L{i}_digests"]
        first = {c: v for v, c in reversed(list(enumerate(L.cams)))}
        same = all(digests[r, v] == digests[0, first[c]] for r in range(L.repeats) for v, c in enumerate(L.cams))
        if not same:
            failures.append((L.label, "views of one camera differ"))
            continue
        bad = []
        y1 = L.y1 if L.y1 is not None else L.size[1]
        for cam, view in zip(data[f"L{i}_cams"], data[f"L{i}_views"]):
            want = _oracle(O, K, L.scene, int(cam), L.encode, L.size)[L.y0:y1]
            rep = diff_report(view, want)
            if rep["mismatched_pixels"] != 0:
                bad.append((int(cam), rep))
            shown = _SHOWN.setdefault(L.scene, [False, False])
            far = _oracle(O, K, L.scene, len(F.CAMERAS) - 1, L.encode, F.FRAME)[0, 0]  # a corner of the far view
            shown[0] |= bool((want == far).all(-1).any())
            shown[1] |= bool((want != far).any(-1).any())
        if bad:
            failures.append((L.label, "pixels differ from the oracle", F.short(F.instantiation(want_tuple, L.scene)), bad))
            continue
        checked.add(F.instantiation(want_tuple, L.scene))
    return checked, failures


def _verified(config, tmp_path_factory, O, K):
    if config not in _RESULTS:
        if _STOPPED:
            pytest.fail(f"not started: {_STOPPED[0][0]} ended with {_STOPPED[0][1]}")
        rc, tail, out = _child(config, tmp_path_factory.mktemp("forms"))
        if rc != 0:
            _STOPPED.append((config, rc))
            _RESULTS[config] = (set(), [f"the child ended with {rc}:\n{tail}"])
        else:
            with np.load(out) as data:
                _RESULTS[config] = _check(config, data, O, K)
            out.unlink()
    return _RESULTS[config]


@pytest.mark.parametrize("config", list(F.CONFIGS))
def test_form(config, tmp_path_factory, oracle, kifs):
    """Every launch of the configuration: the debug tuple it must report, identical views per camera, the oracle's
    bytes."""
    checked, failures = _verified(config, tmp_path_factory, oracle, kifs)
    assert not failures, failures
    assert checked


@pytest.mark.parametrize("name", [F.short(n) for n in F.RENDER_FORMS])
def test_instantiation(name, tmp_path_factory, oracle, kifs):
    """The recipe's configuration rendered its scene on this instantiation (asserted tuple, compared pixels)."""
    full = next(n for n in F.RENDER_FORMS if F.short(n) == name)
    recipe = F.RENDER_FORMS[full]
    if _STOPPED:
        pytest.fail(f"not started: {_STOPPED[0][0]} ended with {_STOPPED[0][1]}")
    checked, failures = _verified(recipe.config, tmp_path_factory, oracle, kifs)
    assert full in checked, (recipe, failures)


def test_every_scene_shows_background_and_fractal(tmp_path_factory, oracle, kifs):
    """Each scene of the table, except the unknown primitive (never hit), shows both in some checked view."""
    if _STOPPED:
        pytest.fail(f"not started: {_STOPPED[0][0]} ended with {_STOPPED[0][1]}")
    for config in F.CONFIGS:
        _verified(config, tmp_path_factory, oracle, kifs)
    for scene in F.SCENES:
        shown = _SHOWN.get(scene)
        assert shown is not None, scene
        assert shown == [True, scene != "unknown"], (scene, shown)
