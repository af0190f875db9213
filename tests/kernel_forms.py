"""The form table: every render kernel instantiation the library compiles, and how a test reaches it on purpose.

The launch rules of kifs_schedule.cpp pick a kernel form per launch from tuned thresholds, so which instantiation a
workload meets is an accident of those thresholds.  Here the KIFS_TUNING=1 knobs force the form instead (their values are
read once per process, so each configuration below runs in a child process of its own: tests/kernel_forms_child.py),
and every instantiation has a RECIPE: the configuration, the scene and the debug tuple

    (debug_last_kernel, debug_last_group_tiles, debug_last_bunny_form, debug_last_round_steps)

the launch must report.  tests/test_kernel_form_coverage.py checks on the CPU that the table's keys are exactly the
instantiations `make report` lists; tests/test_gpu_kernel_forms.py renders every configuration and compares it with
the oracle.  Keys are the demangled names as `make report` prints them.

Nothing here opens the GPU: the parent test process imports this module, builds uniforms and runs the oracle.
"""
from dataclasses import dataclass, field

import numpy as np

KIFS, JULIA, GENJULIA = 0, 1, 2
BUNNY, UNKNOWN = 5, 17  # primitive ids; any id past the bunny is kifs.wgsl's constant-1 SDF (PRIM_OTHER = 6)
PRIM_OTHER = 6
TILE_W, TILE_H = 32, 8
REQUEUE_MIN_WORKGROUPS = 4096  # kifs_schedule.cpp rules::REQUEUE_MIN_WORKGROUPS
MAX_BATCH_INLINE = 64          # kifs_params.hpp

# ---- launch geometry: the same in every configuration, so every form must produce the same bytes ----------------
FRAME = (330, 149)      # 11 x 19 = 209 tiles (odd): the last column is 10 px wide, the last row 5 px high
LONE = (1030, 1032)     # 33 x 129 = 4257 tiles: a lone frame past REQUEUE_MIN_WORKGROUPS on its own
VIEWS = 24              # 4 cameras x 6; 209 x 24 = 5016 workgroups, the band's 176 x 24 = 4224
BIG_VIEWS = 68          # beyond MAX_BATCH_INLINE: the views go through the device table
BAND = (13, 139)        # cuts a tile row at both ends of the frame's grid; its last tile is 6 rows high
LONE_REPEATS = 4        # one feedback period of a lone frame: record costs, sort, adopt the order, a plain launch
SHUFFLE_SEED = 20261016


def tiles(w, h, y0=0, y1=None):
    y1 = h if y1 is None else y1
    return ((w + TILE_W - 1) // TILE_W) * ((y1 - y0 + TILE_H - 1) // TILE_H)


# ---- scenes ------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Scene:
    group: int
    prim: int = 0
    max_iterations: int = 125           # odd: the last round is partial for rounds of 3, 4, 8, 16 and 32 steps
    iters: tuple = (24, 10, 10)         # (sdf_iters, normal_iters, fold_iters)
    constant: tuple = (-0.2, 0.6, 0.2, 0.2)
    power: float = 2.0
    epsilon: float = 1e-4
    max_distance: float = 1000.0
    shadow: bool = False
    encodes: tuple = (1,)               # 1 = sRGB, 0 = UNORM
    fractal_color: tuple = (230, 170, 80)
    background_color: tuple = (12, 24, 48)

    @property
    def bound(self):
        """B of fill_params' bounding sphere (|p| - B <= d(p)); None: no bound, the culls are off."""
        if self.group != KIFS:
            return 2.0
        return {0: 1.0, 1: 2.2360680, 2: 1.7320508, 3: 1.3, 4: 2.0, BUNNY: 1.0}.get(self.prim)


ELIGIBLE_C = (-0.2, 0.6, 0.2, 0.2)      # every |c_i| in [0.1, 1]: far inside the doubled trip's window
INELIGIBLE_C = (-0.2, 0.6, 0.0, 0.2)    # an exact 0.0 component: outside it
SHADOW = dict(shadow_steps=24, shadow_k=8.0, shadow_t0=0.02, shadow_max_t=6.0)

SCENES = {
    "sphere": Scene(KIFS, 0, iters=(24, 10, 5), encodes=(1, 0)),
    "cylinder": Scene(KIFS, 1, iters=(24, 10, 9), encodes=(0,)),
    "box": Scene(KIFS, 2, encodes=(1,)),
    "torus_shadow": Scene(KIFS, 3, iters=(24, 10, 6), shadow=True, encodes=(0,)),
    "sierpinski": Scene(KIFS, 4, iters=(24, 10, 7), encodes=(1,)),      # an odd number of folds
    # the two estimates that read the `lanes` mask the pooled soft-shadow shader hands them (the fold loop, the
    # generalised Julia step), and the bunny shaded through soft_shadow
    "sierpinski_shadow": Scene(KIFS, 4, iters=(24, 10, 7), shadow=True, encodes=(1,)),
    "unknown": Scene(KIFS, UNKNOWN, encodes=(0,)),
    "bunny": Scene(KIFS, BUNNY, max_iterations=61, encodes=(1, 0)),
    "bunny_shadow": Scene(KIFS, BUNNY, max_iterations=61, shadow=True, encodes=(1,)),
    # the four builds of the Julia long-ray loop: bit 1 = the doubled orbit trip, bit 0 = sdf_iters <= 24
    "julia_v0": Scene(JULIA, max_iterations=131, iters=(25, 6, 10), constant=INELIGIBLE_C, encodes=(0,)),
    "julia_v1": Scene(JULIA, max_iterations=131, iters=(24, 6, 10), constant=INELIGIBLE_C, encodes=(1,)),
    "julia_v2_shadow": Scene(JULIA, max_iterations=131, iters=(25, 6, 10), constant=ELIGIBLE_C, shadow=True, encodes=(0,)),
    "julia_v3": Scene(JULIA, max_iterations=131, iters=(24, 6, 10), constant=ELIGIBLE_C, encodes=(1, 0)),
    "genjulia": Scene(GENJULIA, max_iterations=29, iters=(5, 3, 10), power=3.5, constant=(-0.3, 0.5, 0.3, 0.1),
                      encodes=(1,)),
    "genjulia_shadow": Scene(GENJULIA, max_iterations=29, iters=(5, 3, 10), power=3.5, constant=(-0.3, 0.5, 0.3, 0.1),
                             shadow=True, encodes=(0,)),
    # max_iterations exactly 2 x round_steps: the smallest march that is still re-queued
    "sphere_2steps": Scene(KIFS, 0, max_iterations=2, encodes=(1,)),
    "sphere_6steps": Scene(KIFS, 0, max_iterations=6, encodes=(0,)),
}

# Cameras, as multiples of the scene's R = B + epsilon.  The culls use the sphere of radius sqrt(1.1) R (cull_n2), the
# wave-level quick exit sqrt(1.2) R (quick_cull_n2).
CAMERAS = (
    (0.9, 0.4, 0.3),                # inside the bounding sphere: the Julia set may be hit at t = 0
    (1.0488, 2.0, -0.5),            # on it
    (1.0955 * 1.25, 3.7, 0.9),      # just outside the quick-exit sphere: the ring of tiles the tile cull must keep
    (1.0955 * 4.0, 5.1, -0.2),      # far: the projected sphere covers a few tiles, whole tiles are culled
)


def camera(K, scene, index):
    s = SCENES[scene]
    d, phi, theta = CAMERAS[index]
    r = (s.bound if s.bound is not None else 2.0) + s.epsilon
    return K.CameraData(origin_distance=float(d * r), min_distance=0.05, phi=phi, theta=theta)


def options(K, scene):
    """The packed options image of a scene (the unknown primitive id is written into the image directly)."""
    s = SCENES[scene]
    known = s.prim if s.prim <= BUNNY else 0
    u = K.GuiData(max_iterations=s.max_iterations, max_distance=s.max_distance, epsilon=s.epsilon,
                  fractal_color=s.fractal_color, background_color=s.background_color,
                  fractal_group=K.FractalGroup(s.group), primitive_shape=K.PrimitiveShape(known), power=s.power,
                  constant=s.constant).into_buffer_data()
    u.primitive_id = s.prim
    return u


def extensions(scene):
    """Keyword arguments of GraphicState.set_extensions (and of the oracle's Ext)."""
    return dict(soft_shadow=True, **SHADOW) if SCENES[scene].shadow else dict(soft_shadow=False)


# ---- the Julia PRIM slot (launch_render, kifs_kernels.hip) -----------------------------------------------------------
def orbit_x2_eligible(s):
    """kifs_schedule.cpp orbit_x2_eligible(): the doubled orbit trip is exact when every |c_i| lies in [2^-14, 2^10]
    and max_distance and bound_n2 (~ (2 + epsilon)^2) in (0, 2^60].  An exact 0.0 component fails the first test."""
    c = np.float32(s.constant)
    far = 2.0 ** 60
    b2 = float(np.float32(2.0 + s.epsilon)) ** 2
    return bool(np.all((np.abs(c) >= 2.0 ** -14) & (np.abs(c) <= 2.0 ** 10))) and 0 < s.max_distance <= far and 0 < b2 <= far


def prim_slot(scene):
    """The second template argument of the throughput kernels (render_wave_kernel)."""
    s = SCENES[scene]
    if s.group == JULIA:  # bit 1: the doubled orbit trip; bit 0: the short divide / square root (sdf_iters <= 24)
        return (2 if orbit_x2_eligible(s) else 0) | (1 if s.iters[0] <= 24 else 0)
    if s.group == GENJULIA:
        return 0
    return s.prim if s.prim <= BUNNY else PRIM_OTHER


def instantiation(observed, scene):
    """The instantiation a launch ran, from its debug tuple and its scene (launch_render / launch_variant /
    launch_bunny_quad / launch_ssaa).  render_kernel and render_group_kernel take LPRIM = PRIM & 1 for Julia."""
    kernel, group_tiles, bunny_form, _ = observed
    s = SCENES[scene]
    slot = prim_slot(scene)
    lprim = slot & 1 if s.group == JULIA else slot
    if kernel == "render_kernel":
        return f"void kifs::render_kernel<{s.group}, {lprim}>(kifs::BatchParams)"
    if kernel == "render_group_kernel":
        w2lds = "true" if bunny_form == 2 else "false"
        return f"void kifs::render_group_kernel<{s.group}, {lprim}, {group_tiles}, {w2lds}>(kifs::BatchParams)"
    if kernel == "render_wave_kernel":
        return f"void kifs::render_wave_kernel<{s.group}, {slot}>(kifs::BatchParams)"
    if kernel == "render_bunny_quad_kernel":
        return "kifs::render_bunny_quad_kernel(kifs::BatchParams)"
    if kernel == "render_bunny_coop_kernel":
        return "void kifs::render_bunny_coop_kernel<2>(kifs::BatchParams)"
    if kernel == "render_ssaa_kernel":
        return f"void kifs::ssaa::render_kernel<{s.group}, {lprim}>(kifs::BatchParams)"
    raise ValueError(f"unknown kernel {kernel!r}")


# ---- child configurations ----------------------------------------------------------------------------------------
NON_BUNNY = ("sphere", "cylinder", "box", "torus_shadow", "sierpinski", "sierpinski_shadow", "unknown",
             "julia_v0", "julia_v1", "julia_v2_shadow", "julia_v3", "genjulia", "genjulia_shadow")


@dataclass(frozen=True)
class Config:
    knobs: dict                 # KIFS_* knobs besides KIFS_TUNING=1
    scenes: tuple
    extras: dict = field(default_factory=dict)  # launch kind -> scene: "band", "big", "shuffle", "lone" (a tuple)
    timeout: int = 240          # seconds for the child, start-up included


_EXTRAS = dict(band="sierpinski", big="julia_v0", shuffle="box", lone=("julia_v1", "sierpinski"))
_BUNNY_EXTRAS = dict(band="bunny", big="bunny", shuffle="bunny")

CONFIGS = {
    "block": Config({"KIFS_ROUND_STEPS": 0}, NON_BUNNY + ("bunny",), timeout=300),
    "group1": Config({"KIFS_GROUP_TILES": 1}, NON_BUNNY, _EXTRAS),
    "group2": Config({"KIFS_GROUP_TILES": 2}, NON_BUNNY, _EXTRAS),
    "wave": Config({"KIFS_GROUP_TILES": 0}, NON_BUNNY, _EXTRAS),
    "bunny_t1": Config({"KIFS_BUNNY_COOP": 0, "KIFS_GROUP_TILES": 1, "KIFS_ROUND_STEPS": 8}, ("bunny",), _BUNNY_EXTRAS, 300),
    "bunny_t2": Config({"KIFS_BUNNY_COOP": 0, "KIFS_GROUP_TILES": 2, "KIFS_ROUND_STEPS": 8}, ("bunny", "bunny_shadow"), _BUNNY_EXTRAS, 300),
    "bunny_w2lds": Config({"KIFS_BUNNY_COOP": 2, "KIFS_ROUND_STEPS": 8}, ("bunny",), _BUNNY_EXTRAS, 300),
    "bunny_coop": Config({"KIFS_BUNNY_COOP": 1, "KIFS_ROUND_STEPS": 4}, ("bunny", "bunny_shadow"), _BUNNY_EXTRAS, 300),
}
for _rs, _boundary in ((1, "sphere_2steps"), (3, "sphere_6steps")):
    for _form, _tiles in (("group1", 1), ("group2", 2), ("wave", 0)):
        CONFIGS[f"rs{_rs}_{_form}"] = Config({"KIFS_GROUP_TILES": _tiles, "KIFS_ROUND_STEPS": _rs}, NON_BUNNY + (_boundary,))


def child_env(environ, config):
    """The child's environment: `environ` without any KIFS_* variable, plus KIFS_TUNING=1 and the configuration's knobs."""
    env = {k: v for k, v in environ.items() if not k.startswith("KIFS_")}
    env["KIFS_TUNING"] = "1"
    env.update({k: str(v) for k, v in CONFIGS[config].knobs.items()})
    return env


@dataclass(frozen=True)
class Launch:
    label: str
    scene: str
    size: tuple         # (W, H) of the screen
    cams: tuple         # camera index per view
    encode: int
    y0: int = 0
    y1: int = None
    shuffle: bool = False   # debug_set_tile_order with a seeded permutation first
    repeats: int = 1        # lone frames: the same launch several times

    @property
    def rows(self):
        return (self.y1 if self.y1 is not None else self.size[1]) - self.y0


def _cycle(n):
    return tuple(i % len(CAMERAS) for i in range(n))


def plan(config):
    """Every launch of a configuration, in the child's order."""
    c = CONFIGS[config]
    out = []
    for scene in c.scenes:
        for enc in SCENES[scene].encodes:
            out.append(Launch(f"{scene}/{'srgb' if enc else 'unorm'}", scene, FRAME, _cycle(VIEWS), enc))
    if "band" in c.extras:
        s = c.extras["band"]
        out.append(Launch(f"{s}/band", s, FRAME, _cycle(VIEWS), SCENES[s].encodes[0], *BAND))
    if "big" in c.extras:
        s = c.extras["big"]
        out.append(Launch(f"{s}/views{BIG_VIEWS}", s, FRAME, _cycle(BIG_VIEWS), SCENES[s].encodes[-1]))
    for s in c.extras.get("lone", ()):
        out.append(Launch(f"{s}/lone", s, LONE, (0,), SCENES[s].encodes[0], repeats=LONE_REPEATS))
    if "shuffle" in c.extras:  # last: the pinned order stays with the frame's tile table
        s = c.extras["shuffle"]
        out.append(Launch(f"{s}/shuffled", s, FRAME, _cycle(VIEWS), SCENES[s].encodes[0], shuffle=True))
    return out


def shuffled_order(w, h):
    tx, ty = (w + TILE_W - 1) // TILE_W, (h + TILE_H - 1) // TILE_H
    ids = np.array([(j << 16) | i for j in range(ty) for i in range(tx)], dtype=np.uint32)
    return np.random.default_rng(SHUFFLE_SEED).permutation(ids)


# ---- the debug tuple a launch must report --------------------------------------------------------------------------
def expected_tuple(config, launch, scenes=None):
    """The rules of kifs_schedule.cpp (fill_params, enqueue_batch) that remain once the configuration's knobs have forced
    the form: the round length per pipeline (16 Julia / gen-Julia, 8 KIFS and gen-Julia under 32 steps, 32 for a lone
    Julia frame of 64+ steps, 4 for KIFS on one wave per tile), no rounds below 2 x round_steps steps, below
    REQUEUE_MIN_WORKGROUPS workgroups or for a lone bunny frame.  A forced KIFS_ROUND_STEPS replaces every round rule.
    `scenes`: the table `launch.scene` names, when it is not this module's (tests/option_gates.py)."""
    s, knobs = (SCENES if scenes is None else scenes)[launch.scene], CONFIGS[config].knobs
    views = len(launch.cams)
    forced = knobs.get("KIFS_ROUND_STEPS")
    bunny = s.group == KIFS and s.prim == BUNNY
    if forced is not None:
        r = forced
    elif s.group == KIFS or (s.group == GENJULIA and s.max_iterations < 32):
        r = 8
    else:
        r = 16
    if s.max_iterations < 2 * r:
        r = 0
    if forced is None and r == 16 and views == 1 and s.group == JULIA and s.max_iterations >= 64:
        r = 32
    if bunny and views == 1:
        r = 0
    if tiles(*launch.size, launch.y0, launch.y1) * views < REQUEUE_MIN_WORKGROUPS:
        r = 0
    shape = knobs.get("KIFS_GROUP_TILES")
    coop = knobs.get("KIFS_BUNNY_COOP")
    if bunny:
        shape = 2 if coop else shape
    if forced is None and shape == 0 and s.group == KIFS and not bunny and r == 8:
        r = 4
    if r == 0:
        return ("render_bunny_quad_kernel" if bunny else "render_kernel", -1, -1, 0)
    if bunny:
        return ("render_bunny_coop_kernel" if coop == 1 else "render_group_kernel", shape, coop, r)
    return ("render_wave_kernel" if shape == 0 else "render_group_kernel", shape, -1, r)


# ---- the table ------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Recipe:
    config: str
    scene: str
    tuple: tuple    # (kernel, group_tiles, bunny_form, round_steps) of the scene's batched launch


def _recipes():
    t = {}
    kifs_scenes = ("sphere", "cylinder", "box", "torus_shadow", "sierpinski", "unknown")
    for scene in kifs_scenes + ("julia_v0", "julia_v1", "genjulia"):
        rounds = 16 if scene.startswith("julia") else 8
        name = lambda kernel, *a: f"void kifs::{kernel}<{', '.join(str(x) for x in (SCENES[scene].group, prim_slot(scene)) + a)}>(kifs::BatchParams)"
        t[name("render_kernel")] = Recipe("block", scene, ("render_kernel", -1, -1, 0))
        t[name("render_group_kernel", 1, "false")] = Recipe("group1", scene, ("render_group_kernel", 1, -1, rounds))
        t[name("render_group_kernel", 2, "false")] = Recipe("group2", scene, ("render_group_kernel", 2, -1, rounds))
    for scene in kifs_scenes + ("julia_v0", "julia_v1", "julia_v2_shadow", "julia_v3", "genjulia"):
        rounds = 4 if SCENES[scene].group == KIFS else 16 if SCENES[scene].group == JULIA else 8
        t[f"void kifs::render_wave_kernel<{SCENES[scene].group}, {prim_slot(scene)}>(kifs::BatchParams)"] = \
            Recipe("wave", scene, ("render_wave_kernel", 0, -1, rounds))
    t["kifs::render_bunny_quad_kernel(kifs::BatchParams)"] = Recipe("block", "bunny", ("render_bunny_quad_kernel", -1, -1, 0))
    t["void kifs::render_group_kernel<0, 5, 1, false>(kifs::BatchParams)"] = \
        Recipe("bunny_t1", "bunny", ("render_group_kernel", 1, 0, 8))
    t["void kifs::render_group_kernel<0, 5, 2, false>(kifs::BatchParams)"] = \
        Recipe("bunny_t2", "bunny", ("render_group_kernel", 2, 0, 8))
    t["void kifs::render_group_kernel<0, 5, 2, true>(kifs::BatchParams)"] = \
        Recipe("bunny_w2lds", "bunny", ("render_group_kernel", 2, 2, 8))
    t["void kifs::render_bunny_coop_kernel<2>(kifs::BatchParams)"] = \
        Recipe("bunny_coop", "bunny", ("render_bunny_coop_kernel", 2, 1, 4))
    return t


RENDER_FORMS = _recipes()

# ssaa::render_kernel<G, P>: claimed by the case of tests/test_gpu_ssaa.py::test_aa_frame_bit_exact that reaches it
SSAA_FORMS = {
    "void kifs::ssaa::render_kernel<0, 0>(kifs::BatchParams)": "sphere",
    "void kifs::ssaa::render_kernel<0, 1>(kifs::BatchParams)": "cylinder",
    "void kifs::ssaa::render_kernel<0, 2>(kifs::BatchParams)": "box",
    "void kifs::ssaa::render_kernel<0, 3>(kifs::BatchParams)": "torus",
    "void kifs::ssaa::render_kernel<0, 4>(kifs::BatchParams)": "sierpinski",
    "void kifs::ssaa::render_kernel<0, 5>(kifs::BatchParams)": "bunny",
    "void kifs::ssaa::render_kernel<0, 6>(kifs::BatchParams)": "unknown_id",
    "void kifs::ssaa::render_kernel<1, 0>(kifs::BatchParams)": "julia_100",   # sdf_iters 100 > 24
    "void kifs::ssaa::render_kernel<1, 1>(kifs::BatchParams)": "julia_12",
    "void kifs::ssaa::render_kernel<2, 0>(kifs::BatchParams)": "genjulia_p2",
}


# geom::, adaptive::, anim::, accum::, occl:: and light::render_kernel<G, P>, accum::jitter_render_kernel<G, P> and
# accum::carry_render_kernel<G, P> (progressive accumulation), chosen by
# dispatch_pipeline<2>(group, primitive, sdf_iters <= 24): each is claimed by the geometry_cases.PIPELINES name that reaches
# it in test_every_pipeline_bit_exact of tests/test_gpu_geometry.py, test_gpu_adaptive.py, test_gpu_animation.py,
# test_gpu_accumulate.py, test_gpu_accumulate_jitter.py, test_gpu_progressive.py, test_gpu_occlusion.py and
# test_gpu_lighting.py (and in the seeded scenes of tests/extension_fuzz_cases.py, which
# take the same names).  adaptive::classify_kernel is no render form -- it reads a
# geometry plane and marches nothing -- and stays out of the table.
_EXTENSION_PIPELINES = {(0, 0): "sphere", (0, 1): "cylinder", (0, 2): "box", (0, 3): "torus", (0, 4): "sierpinski",
                        (0, 5): "bunny", (0, 6): "unknown_id", (1, 0): "julia_25", (1, 1): "julia_24", (2, 0): "genjulia"}


def _extension_forms(namespace, params, kernel="render_kernel"):
    return {f"void kifs::{namespace}::{kernel}<{g}, {p}>({params})": name for (g, p), name in _EXTENSION_PIPELINES.items()}


GEOMETRY_FORMS = _extension_forms("geom", "kifs::BatchParams")
ADAPTIVE_FORMS = _extension_forms("adaptive", "kifs::adaptive::Params")
ANIMATION_FORMS = _extension_forms("anim", "kifs::anim::Params")
ACCUMULATE_FORMS = _extension_forms("accum", "kifs::accum::Params")
JITTER_FORMS = _extension_forms("accum", "kifs::accum::Params", "jitter_render_kernel")
CARRY_FORMS = _extension_forms("accum", "kifs::accum::CarryParams", "carry_render_kernel")
OCCLUSION_FORMS = _extension_forms("occl", "kifs::occl::Params")
LIGHTING_FORMS = _extension_forms("light", "kifs::light::Params")
EXTENSION_FORMS = {"test_gpu_geometry.py": GEOMETRY_FORMS, "test_gpu_adaptive.py": ADAPTIVE_FORMS,
                   "test_gpu_animation.py": ANIMATION_FORMS, "test_gpu_accumulate.py": ACCUMULATE_FORMS,
                   "test_gpu_accumulate_jitter.py": JITTER_FORMS, "test_gpu_progressive.py": CARRY_FORMS,
                   "test_gpu_occlusion.py": OCCLUSION_FORMS, "test_gpu_lighting.py": LIGHTING_FORMS}


def short(name):
    """`void kifs::render_group_kernel<0, 2, 1, false>(kifs::BatchParams)` -> `render_group_kernel<0,2,1,false>`."""
    return name.split("(")[0].replace("void ", "").replace("kifs::", "").replace(" ", "")
