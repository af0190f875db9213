"""What the four GPU families built on tests/extension_fuzz_cases.py share: the context set-up, the scene's geometry
plane (computed once per scene), the oracle's frame with or without the soft-shadow extension, and the wording of a
failure.  Nothing here opens the GPU by itself; `setup` takes the caller's GraphicState."""
import numpy as np

import extension_fuzz_cases as X
import geometry_reference as GR
from geometry_cases import Raw
from helpers import oracle_uniforms


def describe(i, scene):
    name, family, screen, cam, gui, iters, encode = scene
    return (f"scene {i}: {name}, camera family {family}, {screen.width} x {screen.height}, {cam}, {X.options_of(gui)}, "
            f"iters {iters}, encode {encode}")


def first(bad):
    """'N of M differ; first at (...)' for a boolean array of differences."""
    return f"{int(bad.sum())} of {bad.size} differ; first at {tuple(int(v) for v in np.argwhere(bad)[0])}"


def setup(g, screen, cam, gui, iters, k=1, shadow=None):
    """Everything a context renders a scene with; `shadow`: shadow_candidate's settings or None."""
    g.update_screen_data(screen)
    g.set_camera(cam)
    g.update_options(gui.u if isinstance(gui, Raw) else gui)
    g.set_iters(*iters)
    g.set_extensions(**(shadow or dict(soft_shadow=False)))
    g.set_supersampling(k)


_GEOMETRY = {}


def geometry(O, K, i):
    """(texels (H, W, 4) float32, hit (H, W) bool) of scene i of X.scenes(K) from tests/geometry_reference.c, computed
    once and shared by the test families; leave both unchanged."""
    key = (X.SEED, X.N, i)
    if key not in _GEOMETRY:
        _, _, screen, cam, gui, iters, _ = X.scenes(K)[i]
        geom, hit, _ = GR.geometry_frame(O, K, screen, cam, gui, iters)
        _GEOMETRY[key] = (geom, hit)
    return _GEOMETRY[key]


def shadow_of(O, K, i):
    """The extension's settings scene i runs with: shadow_candidate's where the scene has hits, else None."""
    return X.shadow_candidate(i) if geometry(O, K, i)[1].any() else None


def expected_colour(O, K, screen, cam, gui, iters, encode, shadow=None, y0=0, y1=None):
    """The oracle's frame, with the soft-shadow extension where `shadow` is given."""
    s, c, o = oracle_uniforms(O, K, (screen, cam, gui))
    return O.render(s, c, o, O.iters(*iters), encode=encode, y0=y0, y1=y1, ext=X.oracle_ext(O, shadow))
