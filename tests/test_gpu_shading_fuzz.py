"""light::render_kernel and occl::render_kernel on the seeded scenes of tests/extension_fuzz_cases.py with the lights and
terms of tests/shading_fuzz_cases.py, bit for bit against the models (tests/lighting_reference.c,
tests/occlusion_reference.c): cameras inside, on and between the cull radii, marches of 1-3 steps, heatmaps and the unknown
primitive, under directions of any accepted length, weights above 1, highlights of one channel, every shininess, and
terms of 1 to 16 probes.  Every scene runs lone at k = 1 through both entry points; every third also as a 3-view batch that
mixes camera families, every second of those as a band into a padded pitch -- the lit batches supersampled, the
occlusion batches alternately supersampled without a plane and at k = 1 with a padded plane pitch and stride.  Bytes
exactly, planes by bit pattern with any NaN equal to any NaN, no tolerance; the destinations are the sentinel-filled,
padded ones of tests/test_gpu_lighting.py and tests/test_gpu_occlusion.py, whose helpers assert every sentinel intact.
tests/test_shading_fuzz_cases.py shows on the CPU that these draws exercise the light and the term."""
import numpy as np
import pytest

import extension_fuzz_cases as X
import extension_fuzz_support as S
import lighting_reference as LR
import occlusion_reference as OR
import shading_fuzz_cases as Z
from test_gpu_lighting import _call as lit_call
from test_gpu_occlusion import _call as occlusion_call

pytestmark = pytest.mark.gpu

OK = 0
BATCHES = [i for i in range(X.N) if X.has_batch(i)]


@pytest.fixture(scope="module")
def fgs(kifs):
    g = kifs.GraphicState(0)
    yield g
    g.close()


def _assert_bytes(got, want, what):
    bad = (got != want).any(-1)
    assert not bad.any(), f"{what}: colour: {S.first(bad)}: got {got[bad][0]}, want {want[bad][0]}"


def _assert_plane(got, want, what):
    bad = ~OR.same_bits(got, want)
    assert not bad.any(), (f"{what}: factors: {S.first(bad)}: got {got[bad][0]!r} ({got[bad][0].view(np.uint32):#x}), "
                           f"want {want[bad][0]!r} ({want[bad][0].view(np.uint32):#x})")


def _run(g, scene, k, shadow, call):
    """`call()` on the context set up for the scene; the extension and the supersampling are put back whatever happens."""
    _, _, screen, cam, gui, iters, _ = scene
    S.setup(g, screen, cam, gui, iters, k=k, shadow=shadow)
    try:
        return call()
    finally:
        g.set_extensions(soft_shadow=False)
        g.set_supersampling(1)


@pytest.mark.parametrize("index", range(X.N))
def test_lit_scene(index, fgs, kifs, oracle):
    scene = X.scenes(kifs)[index]
    _, _, screen, cam, gui, iters, encode = scene
    spec, ao = Z.light(index), Z.lit_term(index)
    what = f"{S.describe(index, scene)}; light {spec}, term {ao}"
    shadow = S.shadow_of(oracle, kifs, index)
    r = _run(fgs, scene, 1, shadow, lambda: lit_call(fgs, kifs, spec, ao=ao, encode=encode, cpad=24))
    assert r.st == OK, what
    m = LR.lit_frame(oracle, kifs, screen, cam, gui, iters, spec, ao, X.oracle_ext(oracle, shadow))
    _assert_bytes(r.colour[0], LR.encode(oracle, m.rgb, encode), what)


@pytest.mark.parametrize("index", range(X.N))
def test_occlusion_scene(index, fgs, kifs, oracle):
    scene = X.scenes(kifs)[index]
    _, _, screen, cam, gui, iters, encode = scene
    ao = Z.term(index)
    what = f"{S.describe(index, scene)}; term {ao}"
    shadow = S.shadow_of(oracle, kifs, index)
    r = _run(fgs, scene, 1, shadow, lambda: occlusion_call(fgs, kifs, ao, encode=encode, cpad=24))
    assert r.st == OK, what
    m = OR.occlusion_frame(oracle, kifs, screen, cam, gui, iters, ao, X.oracle_ext(oracle, shadow))
    _assert_bytes(r.colour[0], OR.encode(oracle, m.rgb, encode), what)
    _assert_plane(r.plane[0], m.plane, what)


@pytest.mark.parametrize("index", BATCHES)
def test_lit_batch(index, fgs, kifs, oracle):
    """Three views from three camera families in one supersampled launch; a band case writes rows [y0, y1) only."""
    scene = X.scenes(kifs)[index]
    _, _, screen, cam, gui, iters, encode = scene
    spec, ao, k = Z.light(index), Z.lit_term(index), X.supersampling(index)
    cams = X.batch_cameras(kifs, index, scene, Z.LIT_BATCH_SALT)
    y0, y1 = Z.band(index, screen.height, Z.LIT_BATCH_SALT)
    what = f"{S.describe(index, scene)}; light {spec}, term {ao}, k = {k}, rows {y0}..{y1}"
    shadow = S.shadow_of(oracle, kifs, index)
    r = _run(fgs, scene, k, shadow, lambda: lit_call(fgs, kifs, spec, ao=ao, cams=cams, count=3, y0=y0, y1=y1, encode=encode, cpad=24))
    assert r.st == OK and r.colour.shape[:2] == (3, y1 - y0), what
    for v, c in enumerate(cams):
        want = LR.supersampled_bytes(oracle, kifs, screen, c, gui, iters, spec, k, ao=ao, encode_mode=encode,
                                     ext=X.oracle_ext(oracle, shadow))
        _assert_bytes(r.colour[v], want[y0:y1], f"{what}; view {v} ({c})")


@pytest.mark.parametrize("index", BATCHES)
def test_occlusion_batch(index, fgs, kifs, oracle):
    """Three views in one launch: supersampled without a plane, or at k = 1 with a plane of padded pitch and stride."""
    scene = X.scenes(kifs)[index]
    _, _, screen, cam, gui, iters, encode = scene
    ao, k, plane = Z.term(index), Z.occlusion_batch_k(index), Z.occlusion_batch_has_plane(index)
    cams = X.batch_cameras(kifs, index, scene, Z.OCCLUSION_BATCH_SALT)
    y0, y1 = Z.band(index, screen.height, Z.OCCLUSION_BATCH_SALT)
    what = f"{S.describe(index, scene)}; term {ao}, k = {k}, plane {plane}, rows {y0}..{y1}"
    shadow = S.shadow_of(oracle, kifs, index)
    ext = X.oracle_ext(oracle, shadow)
    r = _run(fgs, scene, k, shadow, lambda: occlusion_call(fgs, kifs, ao, cams=cams, count=3, y0=y0, y1=y1, encode=encode, plane=plane,
                                                          ppad=44, spad=112, cpad=24))
    assert r.st == OK and r.colour.shape[:2] == (3, y1 - y0) and (r.plane is not None) == plane, what
    for v, c in enumerate(cams):
        view = f"{what}; view {v} ({c})"
        if plane:
            m = OR.occlusion_frame(oracle, kifs, screen, c, gui, iters, ao, ext, y0, y1)
            _assert_bytes(r.colour[v], OR.encode(oracle, m.rgb, encode), view)
            _assert_plane(r.plane[v], m.plane, view)
        else:
            want = OR.supersampled_bytes(oracle, kifs, screen, c, gui, iters, ao, k, encode_mode=encode, ext=ext)
            _assert_bytes(r.colour[v], want[y0:y1], view)
