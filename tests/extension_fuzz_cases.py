"""Seeded random scenes for the four extension entry points (supersampling, geometry, adaptive, animation): what
tests/test_gpu_parity_fuzz.py is to the plain path.  Scene i takes pipeline geometry_cases.PIPELINES[i % 10], so every
instantiation of ssaa::, geom::, adaptive:: and anim::render_kernel meets n / 10 scenes, and one of four camera
families, rotated so that every pipeline meets every family:

    0  inside the bounding sphere (origin_distance = R U(0.5, 0.95)): a hit at t = 0 is possible, no cull may fire
    1  on it (exactly R)
    2  between the exact cull radius sqrt(1.1) R and the quick-exit radius sqrt(1.2) R (R U(1.05, 1.09))
    3  from just past sqrt(1.2) R outwards (R U(1.10, 2.5)): some waves of a tile leave, then whole tiles

with R = B + epsilon and B the bound of fill_params (2 where there is none: the unknown primitive id).  Options are drawn
from inside the GUI's ranges; sizes are small and mostly ragged, on both sides of one 64-pixel classify row and of 64
rows.  The module only yields scenes and what is drawn per scene (tests/extension_fuzz_support.py has what the GPU
families share to run them).  Nothing here opens the GPU; tests/test_extension_fuzz_cases.py holds the scenes to the oracle so that no GPU test
passes on empty frames."""
import functools

import numpy as np

import adaptive_reference as AR
from geometry_cases import PIPELINES, Raw

SEED = 20261020  # (20261018 and 20261019 miss the per-pipeline condition of tests/test_extension_fuzz_cases.py)
N = 40
FAMILIES = 4
HEAVY = ("genjulia", "bunny")
# B of fill_params' bounding sphere per pipeline (kifs_schedule.cpp); unknown_id has none
BOUND = {"julia_24": 2.0, "julia_25": 2.0, "genjulia": 2.0, "sphere": 1.0, "cylinder": 2.2360680, "box": 1.7320508,
         "torus": 1.3, "sierpinski": 2.0, "bunny": 1.0, "unknown_id": 2.0}
UNKNOWN_ID = 17
MIN_DISTANCE = 0.05


def family_of(i):
    """Scene i's camera family: pipeline i % 10 meets families (p, p + 3, p + 2, p + 1) mod 4 in its four scenes."""
    return (i + i // 10) % FAMILIES


def is_short_march(i):
    return i % 9 == 4


def is_heatmap(i):
    return i % 6 == 5


def radius(name, gui):
    return BOUND[name] + options_of(gui).epsilon


def options_of(gui):
    """The GuiData a scene's options were packed from (Raw keeps it next to the image)."""
    return gui.gui if isinstance(gui, Raw) else gui


def camera(K, rng, family, R):
    """A camera of `family` for a scene of radius R: phi over the whole circle, theta over +-1.5."""
    d = [lambda: R * rng.uniform(0.5, 0.95), lambda: R, lambda: R * rng.uniform(1.05, 1.09),
         lambda: R * rng.uniform(1.10, 2.5)][family]()
    return K.CameraData(origin_distance=float(d), min_distance=MIN_DISTANCE, phi=float(rng.uniform(0, 2 * np.pi)),
                        theta=float(rng.uniform(-1.5, 1.5)))


def pack(K, name, gui):
    """`gui` as the scene tuple carries it: GuiData, or for unknown_id a Raw image with primitive_id = 17."""
    if name != "unknown_id":
        return gui
    u = gui.into_buffer_data()
    u.primitive_id = UNKNOWN_ID
    raw = Raw(u)
    raw.gui = gui
    return raw


def _group_and_shape(K, name):
    FG, PS = K.FractalGroup, K.PrimitiveShape
    if name.startswith("julia"):
        return FG.JuliaSet, PS.Sphere
    if name == "genjulia":
        return FG.GeneralizedJuliaSet, PS.Sphere
    shape = {"sphere": PS.Sphere, "cylinder": PS.Cylinder, "box": PS.Box, "torus": PS.Torus,
             "sierpinski": PS.SierpinskiTetrahedron, "bunny": PS.Bunny, "unknown_id": PS.Sphere}[name]
    return FG.KaleidoscopicIFS, shape


def _colour(rng):
    return tuple(int(v) for v in rng.integers(0, 256, 3))


@functools.lru_cache(maxsize=None)
def _scenes(K, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        name = PIPELINES[i % len(PIPELINES)]
        heavy = name in HEAVY
        family = family_of(i)
        w = int(rng.integers(17, 57 if heavy else 97))
        h = int(rng.integers(9, 41 if heavy else 73))
        if i % 8 == 1:  # some widths are whole tiles, some heights whole tile rows: the unragged store path
            w = 32 * int(rng.integers(1, 2 if heavy else 4))
        if i % 8 == 6:
            h = 8 * int(rng.integers(2, 6 if heavy else 10))
        if i % 7 == 3:  # lower than 4 k rows for k = 3 and 4 (k = 2 + i % 3 in the adaptive and supersampling families)
            h = int(rng.integers(9, 12))
        steps = int(rng.integers(1, 4)) if is_short_march(i) else int(round(10 ** rng.uniform(np.log10(8), np.log10(50 if heavy else 400))))
        group, shape = _group_and_shape(K, name)
        gui = K.GuiData(
            max_iterations=steps,
            max_distance=float(10 ** rng.uniform(1, 4)),
            epsilon=float(10 ** rng.uniform(-5, -1)),
            fractal_color=_colour(rng), background_color=_colour(rng),
            is_heatmap=is_heatmap(i),
            fractal_group=group, primitive_shape=shape,
            power=float(rng.uniform(1, 10)),
            constant=tuple(float(v) for v in rng.uniform(-1, 1, 4)))
        sdf = {"julia_24": (1, 25), "julia_25": (25, 41), "genjulia": (1, 8)}.get(name, (0, 40))
        iters = (int(rng.integers(*sdf)), int(rng.integers(0, 4 if heavy else 12)), int(rng.integers(0, 24)))
        cam = camera(K, rng, family, BOUND[name] + gui.epsilon)
        out.append((name, family, K.ScreenData(w, h), cam, pack(K, name, gui), iters, int(rng.integers(0, 2))))
    return tuple(out)


def scenes(K, n=N, seed=SEED):
    """[(name, family, screen, camera, gui, iters, encode)]: the same scenes every run."""
    return list(_scenes(K, n, seed))


def scene_rng(i, salt, seed=SEED):
    """The generator a test family draws scene i's extras from (other cameras, thresholds, per-frame options)."""
    return np.random.default_rng([seed, i, salt])


def other_families(i):
    """The two families the extra views of scene i's 3-view batches take their cameras from."""
    f = family_of(i)
    return (f + 1) % FAMILIES, (f + 2 + i // 3 % 2) % FAMILIES


def batch_cameras(K, i, scene, salt):
    """The 3 views of scene i's batch: its own camera and one from each of two other families."""
    name, _, _, cam, gui, _, _ = scene
    rng = scene_rng(i, salt)
    R = radius(name, gui)
    return [cam] + [camera(K, rng, f, R) for f in other_families(i)]


def has_batch(i):
    """About every third scene also runs as a 3-view batch.  With i = 10 d + p the rule is (2 d + p) % 3 == 0: every
    pipeline p has a batch (two where p % 3 == 0), and since k = 2 + (d + p) % 3 the batches of pipelines p % 3 == 0, 1, 2
    run at k = 2, 4, 3.  (tests/test_extension_fuzz_cases.py holds the spread.)"""
    return (i + i // 10) % 3 == 0


def has_band(i):
    """Every second batch of the geometry family is a band into a padded pitch."""
    return has_batch(i) and batch_number(i) % 2 == 0


def batch_number(i):
    """Scene i's place among the scenes with a batch."""
    return sum(has_batch(j) for j in range(i))


def supersampling(i):
    return 2 + i % 3


def thresholds(i):
    """(normal_cos, depth_rel) of scene i in the adaptive family: every pipeline meets all four kinds in its four scenes."""
    kind = (i + 3 * (i // 10)) % 4
    if kind == 3:
        rng = scene_rng(i, 0x7e5)
        return float(rng.uniform(0.5, 0.9999)), float(10 ** rng.uniform(-3, 0))
    return (AR.SILHOUETTE, AR.DEFAULT, AR.ALL_HITS)[kind]


def shadow_candidate(i):
    """The soft-shadow extension's settings for scene i, or None: every fourth scene, heatmaps excepted.  (A family runs
    them only where the scene has hits; i % 4 == 2 is never a heatmap scene's i % 6 == 5.)"""
    if i % 4 != 2 or is_heatmap(i):
        return None
    rng = scene_rng(i, 0x5ad)
    return dict(soft_shadow=True, shadow_steps=int(rng.integers(4, 33)), shadow_k=float(rng.uniform(2, 16)),
                shadow_t0=float(rng.uniform(0.005, 0.05)), shadow_max_t=float(rng.uniform(2, 8)))


def oracle_ext(O, shadow):
    return None if shadow is None else O.Ext(1, shadow["shadow_steps"], shadow["shadow_k"], shadow["shadow_t0"],
                                             shadow["shadow_max_t"])


def dispatch(name, gui, iters):
    """(GROUP, PRIM) of dispatch_pipeline<2>(group, primitive, sdf_iters <= 24): the instantiation a scene reaches."""
    u = gui.into_buffer_data()
    group, prim = int(u.fractal_group_id), int(u.primitive_id)
    if group == 1:
        return 1, int(iters[0] <= 24)
    if group == 2:
        return 2, 0
    return 0, min(prim, 6)


def animation(K, i, scene):
    """Scene i's animated launch: (screen capped at 64 x 48, [(camera, GuiData or Raw)] of 2, 5 or 9 frames, the frame
    whose bytes are also compared with update_options + render).  Per frame a constant, power, both colours and a camera
    family are drawn; in every third sequence one frame's constant has an exact 0.0 component and another a -0.0."""
    name, _, screen, _, gui, _, _ = scene
    rng = scene_rng(i, 0xa17)
    base = options_of(gui)
    count = (2, 5, 9)[i % 3]
    R = radius(name, gui)
    frames = []
    for f in range(count):
        constant = [float(v) for v in rng.uniform(-1, 1, 4)]
        if i % 3 == 1 and f in (1, 3):
            constant[int(rng.integers(0, 4))] = 0.0 if f == 1 else -0.0
        g = K.GuiData(**{**base.__dict__, "constant": tuple(constant), "power": float(rng.uniform(1, 10)),
                         "fractal_color": _colour(rng), "background_color": _colour(rng)})
        frames.append((camera(K, rng, int(rng.integers(0, FAMILIES)), R), pack(K, name, g)))
    return K.ScreenData(min(screen.width, 64), min(screen.height, 48)), frames, int(rng.integers(0, count))
