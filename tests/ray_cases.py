"""The seeded generator of arbitrary rays for the ray-query tests (kifs_trace_rays_async): n rays in five classes,
computed in f64, cast to f32 and shuffled, so that the lanes of a wave hold unrelated origins and direction lengths.
    A 50 %  origin on a shell of radius 2.2 .. 4.0, aimed at a uniform point of the ball of radius 0.9, unit direction
    B 15 %  the same, the direction scaled by one of 0.25, 0.5, 2.0, 3.7
    C 15 %  origin uniform in the ball of radius 1.2 (inside several of the solids), random unit direction
    D 15 %  origin on the shell, random unit direction (most of them miss)
    E  5 %  origin uniform in the ball of radius 3, zero direction: a ray that stands still
The scenes are geometry_cases.cases.

grazing() is a second generator, for the ray-level cull of the ray kernel (rays::never_inside, kifs_rays_kernels.hip): the
cull is applied only for |o|^2 <= 1024 and certifies a miss from the closest approach of the ray's LINE, so its rays
start at distances 2.5, 8, 31.9 and 32.1 -- near, far, and either side of the switch -- and their lines are tangent to a
sphere of radius u * bound, u uniform in 0.3 .. 1.15, where `bound` is the scene's bounding radius (BOUND, the comment in
fill_params of kifs_schedule.cpp): from well inside the solid to just outside the radius the cull stands on.  Direction
lengths 0.5 and 1: with longer directions the march oversteps from these distances and with much shorter ones it runs
out of steps, so nothing hits (measured with the reference alone)."""
import numpy as np

N = 2048
CLASSES = "ABCDE"
SHARES = (0.50, 0.15, 0.15, 0.15, 0.05)
SCALES = (0.25, 0.5, 2.0, 3.7)
# grazing(): the origin distances, the direction lengths, u's range and the bounding radius B of every scene
DISTANCES = (2.5, 8.0, 31.9, 32.1)
LENGTHS = (0.5, 1.0)
TANGENT = (0.3, 1.15)
N_GRAZING = 1600
# The generalised Julia set of the test scene (power 3.5, 64 march steps) is thin and its march short: about 2.5 % of
# these rays hit it (8 to 15 of 400 per distance at 1600 rays, 41 to 63 of 2000 at 8000 over three seeds, the reference
# alone), nearly all of them at length 1.  It gets five times the rays, so that 30 hits per distance are expected twice over.
N_GRAZING_OF = {"genjulia": 8000}
BOUND = {"julia_24": 2.0, "julia_25": 2.0, "genjulia": 2.0, "sphere": 1.0, "cylinder": 5.0 ** 0.5, "box": 3.0 ** 0.5, "torus": 1.3,
         "sierpinski": 2.0, "bunny": 1.0, "unknown_id": 2.0}  # (an unknown id has no bound: the SDF is the constant 1)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _ball(rng, n, radius):
    return _unit(rng, n) * (radius * rng.random(n) ** (1.0 / 3.0))[:, None]


def _shell(rng, n):
    return _unit(rng, n) * rng.uniform(2.2, 4.0, n)[:, None]


def _aimed(rng, n):
    o = _shell(rng, n)
    d = _ball(rng, n, 0.9) - o
    return o, d / np.linalg.norm(d, axis=1, keepdims=True)


def rays(seed, n=N):
    """((n, 8) float32 rays in KifsRay layout, (n,) array of class letters), shuffled with the same generator."""
    rng = np.random.default_rng(seed)
    counts = [int(round(s * n)) for s in SHARES[:-1]]
    counts.append(n - sum(counts))
    parts, labels = [], []
    for c, m in zip(CLASSES, counts):
        if c == "A":
            o, d = _aimed(rng, m)
        elif c == "B":
            o, d = _aimed(rng, m)
            d = d * rng.choice(SCALES, m)[:, None]
        elif c == "C":
            o, d = _ball(rng, m, 1.2), _unit(rng, m)
        elif c == "D":
            o, d = _shell(rng, m), _unit(rng, m)
        else:
            o, d = _ball(rng, m, 3.0), np.zeros((m, 3))
        r = np.zeros((m, 8), dtype=np.float64)
        r[:, 0:3] = o
        r[:, 4:7] = d
        parts.append(r)
        labels += [c] * m
    out = np.concatenate(parts).astype(np.float32)
    order = rng.permutation(n)
    return np.ascontiguousarray(out[order]), np.array(labels)[order]


def grazing(seed, bound, n=N_GRAZING):
    """((n, 8) float32 rays in KifsRay layout, (n,) origin distances, (n,) direction lengths), shuffled with the same
    generator: n / 4 rays per distance of DISTANCES, half of them per length of LENGTHS.  A ray starts at distance D in a
    uniform direction e and runs along -cos(a) e + sin(a) p, p a uniform unit vector perpendicular to e and
    sin(a) = u * bound / D: its line's closest approach to the centre is u * bound.  u is uniform in TANGENT, its upper
    end lowered to 0.95 D / bound where the tangent sphere would reach the origin (the cylinder and the box from 2.5).
    Computed in f64, cast to f32."""
    rng = np.random.default_rng(seed)
    per = n // len(DISTANCES)
    assert per * len(DISTANCES) == n and per % len(LENGTHS) == 0
    dist = np.repeat(np.array(DISTANCES), per)
    length = np.tile(np.repeat(np.array(LENGTHS), per // len(LENGTHS)), len(DISTANCES))
    e = _unit(rng, n)
    p = np.cross(e, _unit(rng, n))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    u = rng.uniform(TANGENT[0], np.minimum(TANGENT[1], 0.95 * dist / bound))
    sin_a = u * bound / dist
    d = -np.sqrt(1.0 - sin_a * sin_a)[:, None] * e + sin_a[:, None] * p
    r = np.zeros((n, 8), dtype=np.float64)
    r[:, 0:3] = e * dist[:, None]
    r[:, 4:7] = d * length[:, None]
    order = rng.permutation(n)
    return np.ascontiguousarray(r.astype(np.float32)[order]), dist[order], length[order]
