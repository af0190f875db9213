"""Scenes, views and launches of tests/test_gpu_julia_cert_cull.py and its child process (julia_cert_cull_child.py).
Nothing here opens the GPU.

SCENES pair every constant, epsilon and frame size of the test with each other so that each value is met and the
non-vacuity condition CAN hold: at least 25 % of the rays today's cull marches must go for both views at distance
>= 2.05.  Whether it can is geometry, not a property of the code -- from distance 2.05 every ray of a frame is marched
today (the camera is inside sqrt(1.1) (2 + epsilon) = 2.098), and the new cull takes the rays beyond the angle
asin(r / 2.05), r = sqrt(1 + 2^-6) rho, from the axis:

    constant, epsilon     rho     r       tan     share of a 16:9 / 5:3 / 2:1 frame outside that circle (uv.y in [-1, 1])
    headline, 1e-4        1.476   1.487   1.054   0.51 / 0.48 / 0.57
    reference, 1e-4       1.680   1.693   1.466   0.245 / 0.195 / 0.33     <- only the 2:1 frame leaves a quarter
    small, 1e-4 / 1e-2    1.054 / 1.323   ...     0.8 / 0.67 and more
    headline, 1e-2        1.729   1.742   1.61    0.16                     <- not paired: no frame of the three has it
    reference, 1e-2       1.927   1.942   2.96    0                        <- nor this

so the reference constant renders the 2:1 frame (96 x 48) and epsilon = 1e-2 goes with the small constant.  From distance
5, and from the skewed view at distance 3, every certified pairing above loses more than a third of today's rays
(test_the_new_cull_is_not_vacuous prints each share).
"""
import hashlib

import numpy as np

TILE_W, TILE_H = 32, 8
REQUEUE_MIN_WORKGROUPS = 4096  # kifs_schedule.cpp rules::REQUEUE_MIN_WORKGROUPS: below it no form is forced
MAX_ITERATIONS = 125

HEADLINE_C = (-0.2, 0.6, 0.2, 0.2)
REFERENCE_C = (-0.1, 0.6, 0.9, -0.3)
SMALL_C = (0.05, 0.0, 0.0, 0.0)
NO_CERT_C = (0.4, -1.9, 0.5, 0.6)    # |c| = 2.1: the escape radius 2.03 is outside the patch sphere; two orbit trips
                                     # leave a set that every view but the one looking away still hits

#          name               constant     sdf_iters  epsilon  (W, H)
SCENES = {
    "headline_256":  (HEADLINE_C,  12,  1e-4, (256, 144)),
    "headline_200":  (HEADLINE_C,  12,  1e-4, (200, 120)),   # ragged: 6.25 x 15 tiles
    "headline_96":   (HEADLINE_C,  12,  1e-4, (96, 48)),     # under 64 rows: the tile-level exit is off
    "reference_96":  (REFERENCE_C, 100, 1e-4, (96, 48)),
    "small_256":     (SMALL_C,     12,  1e-4, (256, 144)),
    "small_200_e2":  (SMALL_C,     12,  1e-2, (200, 120)),
    "nocert_256":    (NO_CERT_C,   2,   1e-4, (256, 144)),
    "nocert_200_e2": (NO_CERT_C,   2,   1e-2, (200, 120)),
}
NORMAL_ITERS, FOLD_ITERS = 10, 10

# views: (distance, phi, theta, kind)
VIEWS = (
    (5.0, 0.4, 0.3, "at"),
    (2.05, 2.0, -0.5, "at"),      # between rho and the old cull radius
    (1.7, 3.7, 0.9, "at"),        # inside the shell, looking at the set
    (1.7, 3.7, 0.9, "away"),      # and away from it
    (1.0, 5.1, -0.2, "at"),       # inside rho
    (3.0, 1.1, 0.2, "skew"),      # a matrix that is not orthonormal
)
ORTHONORMAL = (0, 1, 2, 3, 4)
WITH_SKEW = (5, 0, 1)


class Image:
    """A uniform image where the helpers expect an object with into_buffer_data()."""
    def __init__(self, u):
        self.u = u

    def into_buffer_data(self):
        return self.u


def view(K, index):
    d, phi, theta, kind = VIEWS[index]
    u = K.CameraData(origin_distance=d, min_distance=0.05, phi=phi, theta=theta).into_buffer_data()
    if kind == "away":      # the forward axis is -matrix[0]
        for k in range(3):
            u.matrix[0][k] = -u.matrix[0][k]
    elif kind == "skew":
        for k in range(3):
            u.matrix[1][k] = 1.3 * u.matrix[1][k] + 0.2 * u.matrix[2][k]
    return Image(u)


def options(K, scene, constant=None):
    c, _, eps, _ = SCENES[scene]
    return K.GuiData(max_iterations=MAX_ITERATIONS, max_distance=1000.0, epsilon=eps, fractal_color=(230, 170, 80),
                     background_color=(12, 24, 48), fractal_group=K.FractalGroup(1),
                     constant=constant if constant is not None else c)


def iters(scene):
    return (SCENES[scene][1], NORMAL_ITERS, FOLD_ITERS)


def tiles(w, h):
    return ((w + TILE_W - 1) // TILE_W) * ((h + TILE_H - 1) // TILE_H)


def launches():
    """(scene, view indices) of every batched launch, each with enough views for REQUEUE_MIN_WORKGROUPS workgroups -- below
    it every launch takes render_kernel whatever the knobs say.  96 x 48 needs 228 views: through the device view table."""
    out = []
    for scene, (_, _, _, size) in SCENES.items():
        need = -(-REQUEUE_MIN_WORKGROUPS // tiles(*size))
        for base in (ORTHONORMAL, WITH_SKEW):
            n = -(-need // len(base)) * len(base)
            out.append((scene, tuple(base[i % len(base)] for i in range(n))))
    return out


# knobs besides KIFS_TUNING=1; each form also runs with KIFS_JULIA_CERT_CULL=0 ("..._off")
FORMS = {
    "block": ({"KIFS_ROUND_STEPS": 0}, ("render_kernel", -1)),
    "group1": ({"KIFS_GROUP_TILES": 1}, ("render_group_kernel", 1)),
    "group2": ({"KIFS_GROUP_TILES": 2}, ("render_group_kernel", 2)),
    "wave": ({"KIFS_GROUP_TILES": 0}, ("render_wave_kernel", 0)),
}


def child_env(environ, form, switch_on):
    env = {k: v for k, v in environ.items() if not k.startswith("KIFS_")}
    env["KIFS_TUNING"] = "1"
    env.update({k: str(v) for k, v in FORMS[form][0].items()})
    if not switch_on:
        env["KIFS_JULIA_CERT_CULL"] = "0"
    return env


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the other entry points: the headline scene at 256 x 144 --------------------------------------------------------
EXTRA_SCENE = "headline_256"
BAND = (13, 139)
ANIMATIONS = (          # constants per frame: one without a certificate first; two with different radii
    (NO_CERT_C, HEADLINE_C),
    (SMALL_C, REFERENCE_C),
)
ACCUMULATE_VIEWS = ((5.0, 0.40, 0.3), (5.0, 0.43, 0.3), (5.0, 0.46, 0.3), (5.0, 0.49, 0.3))  # 4 sub-frames of one frame
