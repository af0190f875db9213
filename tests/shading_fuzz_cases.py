"""What the lit and the occlusion families draw per scene of tests/extension_fuzz_cases.py (the same 40 scenes, the same
seed, scene_rng with salts of their own): a light, an occlusion term, and for the scenes with a batch its three cameras,
its band and its supersampling factor.  The hand-picked scenes of tests/test_gpu_lighting.py and
tests/test_gpu_occlusion.py meet three lights and two terms from one camera outside the bounding sphere; here every
pipeline meets cameras inside, on and between the cull radii, marches of 1-3 steps and heatmaps with

    light(i)   a direction of any length the entry point accepts -- a unit vector (normalised in f64, rounded to f32) in
               three scenes of five, so that the direct term is partial, times 10^U(-18, -2) in one and 10^U(1, 18) in one:
               the direct term takes the direction as given, the shadow ray and the highlight its unit vector, and only a
               direction that is no unit vector tells the two apart --, weights up to 0.5 (ambient) and 1.5 (diffuse: above
               1 channels saturate in the encode) with exact zeros, no highlight in every fourth scene (i % 4 == 3), a
               highlight of ONE channel in every fourth (i % 4 == 2; device_light ORs the three into one flag), and
               every shininess_log2 0..10
    term(i)    1, 16 and 2..15 probes, decay exactly 1, strength exactly 0; the lit family passes NULL in every third scene

Nothing here opens the GPU; tests/test_shading_fuzz_cases.py holds the draws to the models so that no GPU test passes
with the light or the term unseen."""
import numpy as np

import extension_fuzz_cases as X

N = X.N
LIGHT_SALT, TERM_SALT, LIT_BATCH_SALT, OCCLUSION_BATCH_SALT = 0x13f, 0x199, 0x1b7, 0x0b7
UNIT, SMALL, LARGE = 0, 1, 2
# (of the salts 0x100..0x1b3 the light's is the first that meets every condition of tests/test_shading_fuzz_cases.py; three
# of them do for the term -- 0x162, 0x183 and this one, which leaves the most pixels with a partial factor.  0x11c and
# 0xa0c, the first tried, miss several conditions.)


def scale_class(i):
    """Three scenes in five take the unit vector itself, one a short and one a long direction; rotated by the decade so
    that every pipeline meets four of the five places."""
    return (UNIT, UNIT, UNIT, SMALL, LARGE)[(i + i // 10) % 5]


def one_channel(i):
    """The specular's one non-zero channel in the scenes that have just one, else None."""
    return (i // 4) % 3 if i % 4 == 2 else None


def light(i):
    """Scene i's light, as the keyword arguments of lighting_reference.make_light."""
    rng = X.scene_rng(i, LIGHT_SALT)
    v = rng.normal(size=3)
    unit = (v / np.linalg.norm(v)).astype(np.float32)
    exponent = {UNIT: 0.0, SMALL: rng.uniform(-18, -2), LARGE: rng.uniform(1, 18)}[scale_class(i)]
    # (the product is taken in f64 and rounded once; at scale 1 it is the unit vector's own f32 image)
    direction = (unit.astype(np.float64) * 10.0 ** exponent).astype(np.float32)
    ambient, diffuse = float(rng.uniform(0, 0.5)), float(rng.uniform(0, 1.5))
    if i % 13 == 5:
        ambient = 0.0
    if i % 13 == 7:
        diffuse = 0.0
    specular = [float(s) for s in rng.uniform(0, 1, 3)]
    if i % 4 == 3:
        specular = [0.0, 0.0, 0.0]
    elif one_channel(i) is not None:
        specular = [s if c == one_channel(i) else 0.0 for c, s in enumerate(specular)]
    return dict(direction=tuple(float(d) for d in direction), ambient=ambient, diffuse=diffuse, specular=tuple(specular),
                shininess_log2=i % 11)


def term(i):
    """Scene i's occlusion term (samples, step, decay, strength)."""
    rng = X.scene_rng(i, TERM_SALT)
    samples = int(rng.integers(2, 16))
    step, decay, strength = float(10 ** rng.uniform(-3, -0.5)), float(rng.uniform(0.3, 1)), float(rng.uniform(0, 8))
    if i % 13 == 2:
        samples = 1
    if i % 13 == 6:
        samples = 16
    if i % 13 == 10:
        decay = 1.0
    if i == 12:
        strength = 0.0
    return samples, step, decay, strength


def lit_term(i):
    """The term the lit family carries in scene i: two scenes of three, NULL in the third."""
    return term(i) if i % 3 != 2 else None


def band(i, h, salt):
    """Rows [y0, y1) of a band case, neither end a multiple of 8 (frames are at least 9 rows high); the whole frame where
    scene i's batch is no band."""
    if not X.has_band(i):
        return 0, h
    rng = X.scene_rng(i, salt ^ 0xba4d)
    y0 = int(rng.integers(1, min(8, h - 1)))
    return y0, int(rng.choice([y for y in range(y0 + 1, h + 1) if y % 8]))


def occlusion_batch_has_plane(i):
    """The occlusion batches alternate between the scene's supersampling factor without a plane and k = 1 with one (a
    resolved pixel has no single factor); in pairs, so that bands -- every second batch -- meet both."""
    return X.batch_number(i) % 4 in (1, 2)


def occlusion_batch_k(i):
    return 1 if occlusion_batch_has_plane(i) else X.supersampling(i)
