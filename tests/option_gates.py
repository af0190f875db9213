"""The gate table: scenes on both sides of every constant by which kifs_schedule.cpp turns the uniform images into
permissions for the kernels' fast paths (fill_params' `sane` and rounds, orbit_x2_eligible, julia_cull_radius,
set_culls' 64 rows, fill_views' far origin).  kifs_set_options refuses nothing but a group id above 2, so every value
here reaches those gates; the GUI's ranges (max_distance <= 1e4, epsilon in [1e-6, 1], c in [-1, 1]^4, power in
[1, 10], max_iterations >= 1) lie far inside all of them.

A case is a kernel_forms.Scene plus the gate it belongs to, the side of the gate it is on, the pipeline it runs on and
what the oracle shows of it.  gate_sides() restates the host's gates in Python -- tests/test_option_gates_plan.py checks
with it that every gate has a case on each side, tests/hip_stub/host_driver.cpp (GATE_CASES) pins the host's own
decisions on the CPU, tests/test_gpu_option_gates.py renders every case against the oracle.  The module also serves
tests/kernel_forms_child.py in place of kernel_forms (plan, SCENES, options, camera, extensions).

Caps that keep every launch short, whatever a case does to the march: |max_iterations| <= 256, sdf_iters <= 40,
normal_iters <= 12, fold_iters <= 24, shadow_steps <= 32 (no case has shadows).

Nothing here opens the GPU.
"""
from dataclasses import dataclass, replace

import numpy as np

import kernel_forms as F
from kernel_forms import GENJULIA, JULIA, KIFS

f32 = np.float32
NAN, INF = float("nan"), float("inf")


def below(x):
    """The f32 neighbour of f32(x) towards zero, as a Python float."""
    return float(np.nextafter(f32(x), f32(0.0)))


def above(x):
    return float(np.nextafter(f32(x), f32(np.inf)))


SANE_FAR = float(f32(1.0e15))      # fill_params: max_distance < 1.0e15f; fill_views: |origin|^2 < 1e30 (in double)
X2_LO, X2_HI, X2_FAR = 2.0 ** -14, 2.0 ** 10, 2.0 ** 60  # orbit_x2_eligible
TILE_CULL_ROWS = 64                # set_culls
CAPS = dict(max_iterations=256, sdf_iters=40, normal_iters=12, fold_iters=24)

GATES = {
    "E": "fill_params: epsilon >= 0 for the culls, epsilon > 0 for the rounds",
    "R": "fill_params / julia_cull_radius: 0.5 < B + epsilon < 1e6",
    "D": "fill_params / julia_cull_radius: max_distance < 1e15",
    "X": "orbit_x2_eligible: |c_i| in [2^-14, 2^10], max_distance in (0, 2^60]",
    "M": "fill_params: rounds for max_iterations >= 2 x rounds (8 <-> 16 at 32 steps, 32 for a lone frame from 64); "
         "the quick cull for max_iterations > 0",
    "I": "the iteration counts: the Julia orbit's blocks of six trips and its remainder, no trips at all",
    "P": "the generalised Julia set's power",
    "O": "fill_views: |origin|^2 < 1e30",
    "H": "set_culls: the tile cull from 64 rows",
    "S": "screens of a few pixels, whole and ragged tiles",
}


@dataclass(frozen=True)
class Case(F.Scene):
    gate: str = ""
    pipeline: str = ""
    side: str = ""              # "below" / "at" / "above" the gate's constant, or "inside" (the GUI's range)
    heatmap: bool = False
    origin: float = None        # O: |origin| of the raw camera images (on an axis: camera())
    size: tuple = F.FRAME
    views: int = F.VIEWS
    lone: bool = False          # M 63 / 64: a lone frame of kernel_forms.LONE
    shows: str = "fractal"      # or "background_only": from the oracle, recomputed by tests/test_option_gates_plan.py

    @property
    def camera_radius(self):
        """R = B + epsilon; B + 1e-4 where epsilon is not a positive finite number."""
        eps = self.epsilon if (np.isfinite(self.epsilon) and self.epsilon > 0.0) else 1e-4
        return self.bound + eps


# ---- the pipelines -----------------------------------------------------------------------------------------------------
PIPELINES = {
    "julia_24": Case(JULIA, max_iterations=131, iters=(24, 6, 10), constant=F.ELIGIBLE_C, pipeline="julia_24"),
    "julia_25": Case(JULIA, max_iterations=131, iters=(25, 6, 10), constant=F.ELIGIBLE_C, pipeline="julia_25"),
    "genjulia": Case(GENJULIA, max_iterations=29, iters=(5, 3, 10), power=3.5, constant=(-0.3, 0.5, 0.3, 0.1),
                     pipeline="genjulia"),
    "sphere": Case(KIFS, 0, iters=(24, 10, 5), pipeline="sphere"),
    "sierpinski": Case(KIFS, 4, iters=(24, 10, 7), pipeline="sierpinski"),
}

SCENES = {}


def _add(gate, pipeline, label, side, **changes):
    name = f"{gate}/{pipeline}/{label}"
    assert name not in SCENES, name
    SCENES[name] = replace(PIPELINES[pipeline], gate=gate, side=side, **changes)


def _c(i, v):
    c = list(F.ELIGIBLE_C)
    c[i] = v
    return tuple(c)


def _build():
    # E: epsilon's sign.  A negative or NaN epsilon hits nothing (d < epsilon is false for every d >= 0): that side of
    # the gate is background by construction; at 0.0 only a camera inside the solid hits.
    for p in ("julia_24", "genjulia", "sphere", "sierpinski"):
        _add("E", p, "eps=1e-6", "above", epsilon=1e-6)
        _add("E", p, "eps=0", "at", epsilon=0.0)
        _add("E", p, "eps=-1e-3", "below", epsilon=-1e-3)
        _add("E", p, "eps=nan", "below", epsilon=NAN)
    # R: B + epsilon against 1e6 (B = 1: 999999 and 1000001; B = 2: 999999, 1000000 and 1000002), max_distance 1e8 so that
    # rays from 1.05 R get there; 0.6 and 1.0 are large but sane.
    for p in ("sphere", "julia_24"):
        _add("R", p, "eps=0.6", "inside", epsilon=0.6)
        _add("R", p, "eps=1.0", "inside", epsilon=1.0)
        _add("R", p, "eps=999998", "below" if p == "sphere" else "at", epsilon=999998.0, max_distance=1e8)
        _add("R", p, "eps=1e6", "above", epsilon=1e6, max_distance=1e8)
    _add("R", "julia_24", "eps=999997", "below", epsilon=999997.0, max_distance=1e8)
    for label, side, v in (("eps=0.6", "inside", 0.6), ("eps=999997", "below", 999997.0), ("eps=999998", "at", 999998.0)):
        _add("R", "sierpinski", label, side, epsilon=v, max_distance=1e8 if v > 1 else 1000.0)  # B = 2 on the generic loop
    # D: max_distance against 1e15.  NaN and 0.0 let no ray set out (t < max_distance is never true): background by
    # construction.
    for p in ("julia_24", "julia_25", "genjulia", "sphere", "sierpinski"):
        _add("D", p, "md=1e4", "inside", max_distance=1e4)
        _add("D", p, "md<1e15", "below", max_distance=below(SANE_FAR))
        _add("D", p, "md=1e15", "at", max_distance=SANE_FAR)
        _add("D", p, "md=inf", "above", max_distance=INF)
        _add("D", p, "md=nan", "above", max_distance=NAN)
        _add("D", p, "md=0", "inside", max_distance=0.0)
    # X: the doubled trip's window.  At max_distance 2^60 the doubled trip is allowed and the culls are off: the
    # throughput kernel's out-of-line general square root with the x2 trip.
    for p in ("julia_24", "julia_25"):
        _add("X", p, "cx=2^-14", "at", constant=_c(0, X2_LO))
        _add("X", p, "cx<2^-14", "below", constant=_c(0, below(X2_LO)))
        _add("X", p, "cy=2^10", "at", constant=_c(1, X2_HI))
        _add("X", p, "cy>2^10", "above", constant=_c(1, above(X2_HI)))
        _add("X", p, "cz=+0", "below", constant=_c(2, 0.0))
        _add("X", p, "cz=-0", "below", constant=_c(2, -0.0))
        _add("X", p, "md=2^60", "at", max_distance=X2_FAR)
        _add("X", p, "md>2^60", "above", max_distance=above(X2_FAR))
        _add("X", p, "cw=-2^-14", "at", constant=_c(3, -X2_LO))          # the window is one of |c_i|
        _add("X", p, "cw>-2^-14", "below", constant=_c(3, -below(X2_LO)))
    # M: the march budget.  No ray sets out with max_iterations <= 0 (the step count is compared as a signed integer in
    # every march loop: `0 < P.max_iterations`, `trips < limit`, s_cmp_lt_i32): background by construction, the heatmap
    # included (0 / 0 and 0 / -5 steps).
    for p in ("julia_24", "genjulia", "sierpinski"):  # (the generalised Julia set marches in generic_loop, like KIFS)
        for mi in (0, -5) if p != "sierpinski" else (0,):
            _add("M", p, f"mi={mi}", "below", max_iterations=mi)
            _add("M", p, f"mi={mi}/heatmap", "below", max_iterations=mi, heatmap=True)
    for p, pairs in (("sphere", ((15, 16),)), ("sierpinski", ((15, 16),)), ("julia_24", ((31, 32),)),
                     ("genjulia", ((15, 16), (31, 32)))):
        for lo, hi in pairs:
            # (15 steps reach the generalised Julia set only with a wider epsilon; 1e-2 is in the GUI's range)
            wide = dict(epsilon=1e-2) if (p, hi) == ("genjulia", 16) else {}
            _add("M", p, f"mi={lo}", "below", max_iterations=lo, **wide)
            _add("M", p, f"mi={hi}", "at", max_iterations=hi, **wide)
    _add("M", "julia_24", "mi=63/lone", "below", max_iterations=63, lone=True, size=F.LONE, views=1)
    _add("M", "julia_24", "mi=64/lone", "at", max_iterations=64, lone=True, size=F.LONE, views=1)
    # I: iteration counts
    # (the orbit loop takes its blocks of six trips in pairs: 6 and 18 leave one block over, 12 none)
    for n in (0, 1, 5, 6, 7, 12, 18):
        _add("I", "julia_24", f"sdf={n}", "below" if n < 6 else "at" if n == 6 else "above", iters=(n, 6, 10))
    for n in (0, 1):
        _add("I", "genjulia", f"sdf={n}", "below" if n == 0 else "at", iters=(n, 3, 10))
    _add("I", "sierpinski", "fold=0", "below", iters=(24, 10, 0))
    _add("I", "sphere", "normal=0", "below", iters=(24, 0, 5))
    # P: the power
    for label, side, v in (("p=1", "at", 1.0), ("p=10", "at", 10.0), ("p=0", "below", 0.0), ("p=-2", "below", -2.0),
                           ("p=nan", "above", NAN)):
        _add("P", "genjulia", label, side, power=v)
    # O: the origin against 1e15, max_distance below 1e15: f32(1e15)^2 < 1e30 <= above(f32(1e15))^2 in double
    for p in ("julia_24", "sphere"):
        _add("O", p, "origin<1e15", "below", origin=SANE_FAR, max_distance=below(SANE_FAR))
        _add("O", p, "origin>1e15", "above", origin=above(SANE_FAR), max_distance=below(SANE_FAR))
    # H: 88 tiles x 48 views = 4224 workgroups >= REQUEUE_MIN_WORKGROUPS
    for p in ("julia_24", "sierpinski"):
        _add("H", p, "rows=63", "below", size=(330, TILE_CULL_ROWS - 1), views=48)
        _add("H", p, "rows=64", "at", size=(330, TILE_CULL_ROWS), views=48)


_build()

# S: the screens, each lone and as a 3-view batch (tests/test_gpu_option_gates.py)
SCREENS = ((1, 1), (1, 9), (33, 1), (2, 2), (31, 7), (32, 8), (33, 9))
SCREEN_PIPELINES = ("julia_24", "sierpinski")
for _p in SCREEN_PIPELINES:
    for _w, _h in SCREENS:
        SCENES[f"S/{_p}/{_w}x{_h}"] = replace(PIPELINES[_p], gate="S", side="inside", size=(_w, _h), views=3)

# What the oracle shows of each case at 96 x 64 over the four cameras (tests/test_option_gates_plan.py recomputes it):
# every case not named here shows the fractal (>= 1 % of a view off the background, >= 8 colours).  Why these are empty:
#   E eps < 0, NaN  d < epsilon is false for every estimate d >= 0: that side of the gate is empty by construction
#   E eps = 0       only a camera inside the solid hits (d < 0 at its first step): one flat colour
#   D nan, 0        t < max_distance is never true: no ray sets out
#   D inf           the Julia orbits never leave their loop at |q|^2 > max_distance and overflow; KIFS is unchanged
#   X cy = 2^10     |c| = 1024: the set lies far outside the patch sphere of radius 2
#   M <= 0          no step to make: that side of the gate is empty by construction, the heatmap included
#   P 1, 0, NaN     power 1 escapes nothing, 0 gives one flat colour, NaN no hit
#   O               a solid of radius 2 seen from 1e15 is far below one pixel
BACKGROUND_ONLY = {
    "E/julia_24/eps=0", "E/julia_24/eps=-1e-3", "E/julia_24/eps=nan", "E/genjulia/eps=0", "E/genjulia/eps=-1e-3",
    "E/genjulia/eps=nan", "E/sphere/eps=0", "E/sphere/eps=-1e-3", "E/sphere/eps=nan", "E/sierpinski/eps=0",
    "E/sierpinski/eps=-1e-3", "E/sierpinski/eps=nan", "D/julia_24/md=inf", "D/julia_24/md=nan", "D/julia_24/md=0",
    "D/julia_25/md=inf", "D/julia_25/md=nan", "D/julia_25/md=0", "D/genjulia/md=inf", "D/genjulia/md=nan",
    "D/genjulia/md=0", "D/sphere/md=nan", "D/sphere/md=0", "D/sierpinski/md=nan", "D/sierpinski/md=0",
    "X/julia_24/cy=2^10", "X/julia_24/cy>2^10", "X/julia_25/cy=2^10", "X/julia_25/cy>2^10", "M/julia_24/mi=0",
    "M/julia_24/mi=0/heatmap", "M/julia_24/mi=-5", "M/julia_24/mi=-5/heatmap", "M/genjulia/mi=0",
    "M/genjulia/mi=0/heatmap", "M/genjulia/mi=-5", "M/genjulia/mi=-5/heatmap", "M/sierpinski/mi=0",
    "M/sierpinski/mi=0/heatmap", "P/genjulia/p=1", "P/genjulia/p=0", "P/genjulia/p=nan", "O/julia_24/origin<1e15",
    "O/julia_24/origin>1e15", "O/sphere/origin<1e15", "O/sphere/origin>1e15",
}
for _n in BACKGROUND_ONLY:
    SCENES[_n] = replace(SCENES[_n], shows="background_only")


# ---- the host's gates, restated -------------------------------------------------------------------------------------------
def _squared_threshold(T):
    """kifs_schedule.cpp squared_threshold() as far as the gates need it: NaN and +inf -> +inf, negative -> -1."""
    T = f32(T)
    if np.isnan(T) or T == f32(np.inf):
        return INF
    if T < 0:
        return -1.0
    return float(T) * float(T)  # (within an ulp; the gate compares it with 0 and 2^60)


def gate_sides(case, rows=None):
    """(culls on, quick cull on, tile cull on, orbit_x2, round_steps) of a launch of the case without tuning knobs:
    fill_params, set_culls, julia_culls, orbit_x2_eligible and fill_views of kifs_schedule.cpp, in f32 where they are.
    round_steps is fill_params' value, before enqueue_batch's rules on the launch's size (kernel_forms.expected_tuple)."""
    with np.errstate(all="ignore"):
        eps, md = f32(case.epsilon), f32(case.max_distance)
        B = f32(case.bound if case.bound is not None else -1.0)
        R = B + eps
        sane = bool(B > 0 and R > f32(0.5) and R < f32(1.0e6) and eps >= 0 and md < f32(1.0e15))
        quick = sane and not case.heatmap and case.max_iterations > 0
        rows = case.size[1] if rows is None else rows
        tile = quick and rows >= TILE_CULL_ROWS
        if case.origin is not None and not (float(f32(case.origin)) ** 2 < 1.0e30):
            sane = quick = tile = False
        c = np.abs(np.asarray(case.constant, dtype=f32))
        bound_n2 = _squared_threshold(f32(2.0) + eps)
        x2 = bool(np.all((c >= f32(X2_LO)) & (c <= f32(X2_HI)))) and bool(0 < md <= f32(X2_FAR)) and 0 < bound_n2 <= X2_FAR
        r = 16 if case.group != KIFS else 8
        if case.group == GENJULIA and case.max_iterations < 32:
            r = 8
        if case.heatmap or not (eps > 0) or case.max_iterations < 2 * r:
            r = 0
    return sane, quick, tile, x2, r


def caps_hold(case):
    return (abs(case.max_iterations) <= CAPS["max_iterations"] and case.iters[0] <= CAPS["sdf_iters"] and
            case.iters[1] <= CAPS["normal_iters"] and case.iters[2] <= CAPS["fold_iters"] and not case.shadow)


# ---- what tests/kernel_forms_child.py asks of its module -------------------------------------------------------------
CAMERAS = F.CAMERAS
FAR_CAMERAS = (2, 3)
CONFIGS = {k: F.CONFIGS[k] for k in ("block", "group1", "group2", "wave")}
CHILD_GATES = "ERDXMIPOH"
WAVE_GATES = "ERDXOH"   # where the gate can matter on one wave per tile; the other gates run there as well


class RawCamera:
    """A camera image passed where the library's wrappers expect CameraData."""

    def __init__(self, u):
        self.u = u

    def into_buffer_data(self):
        return self.u


def camera(K, scene, index):
    s = SCENES[scene]
    d, phi, theta = CAMERAS[index]
    if s.origin is None:
        return K.CameraData(origin_distance=float(d * s.camera_radius), min_distance=0.05, phi=phi, theta=theta)
    # O: the image of a unit camera a quarter turn per index on, its origin scaled to s.origin in f32.  The origin lies
    # on an axis up to the rounding of cos(pi / 2), 1e-7: |origin|^2 moves by 1e-14 of itself, the two sides of the gate are
    # 1e-7 apart (tests/test_option_gates_plan.py checks the side of every image)
    u = K.CameraData(origin_distance=1.0, min_distance=0.05, phi=float(index) * float(np.pi) / 2.0, theta=0.0).into_buffer_data()
    for k in range(3):
        u.origin[k] = float(f32(u.origin[k]) * f32(s.origin))
    return RawCamera(u)


def options(K, scene):
    """The packed options image: the GUI type's image of an ordinary scene, with every field the case changes written
    into the image directly (the GUI type holds no negative step count; NaN and infinity go the same way)."""
    s = SCENES[scene]
    u = K.GuiData(max_iterations=1, max_distance=1000.0, epsilon=1e-4, fractal_color=s.fractal_color,
                  background_color=s.background_color, fractal_group=K.FractalGroup(s.group),
                  primitive_shape=K.PrimitiveShape(s.prim), power=2.0, constant=(0.0, 0.0, 0.0, 0.0)).into_buffer_data()
    u.max_iterations = int(s.max_iterations)
    u.max_distance = s.max_distance
    u.epsilon = s.epsilon
    u.power = s.power
    u.is_heatmap = 1 if s.heatmap else 0
    for k in range(4):
        u.constant[k] = s.constant[k]
    return u


def extensions(scene):
    return dict(soft_shadow=False)


def names(gates, pipelines=None):
    return [n for n, s in SCENES.items() if s.gate in gates and (pipelines is None or s.pipeline in pipelines)]


def plan(config):
    """Every launch of a configuration, in the child's order: each case of E, R, D, X, M, I, P, O and H as a batch of its
    views (H: the far cameras), the M 63 / 64 pair as lone frames from inside the bounding sphere."""
    out = []
    for name in names(CHILD_GATES):
        s = SCENES[name]
        if s.lone:
            cams = (0,)
        elif s.gate == "H":
            cams = tuple(FAR_CAMERAS[i % 2] for i in range(s.views))
        else:
            cams = tuple(i % len(CAMERAS) for i in range(s.views))
        out.append(F.Launch(name, name, s.size, cams, s.encodes[0]))
    return out


def expected_tuple(config, launch):
    """kernel_forms.expected_tuple plus what it does not know: no rounds with !(epsilon > 0) or a heatmap, in any
    configuration (a budget below 2 x rounds it knows)."""
    s = SCENES[launch.scene]
    if s.heatmap or not (f32(s.epsilon) > 0):
        return ("render_kernel", -1, -1, 0)
    return F.expected_tuple(config, launch, SCENES)
