"""The seeded generator of arbitrary rays for the ray-query tests (kifs_trace_rays_async): n rays in five classes,
computed in f64, cast to f32 and shuffled, so that the lanes of a wave hold unrelated origins and direction lengths.
    A 50 %  origin on a shell of radius 2.2 .. 4.0, aimed at a uniform point of the ball of radius 0.9, unit direction
    B 15 %  the same, the direction scaled by one of 0.25, 0.5, 2.0, 3.7
    C 15 %  origin uniform in the ball of radius 1.2 (inside several of the solids), random unit direction
    D 15 %  origin on the shell, random unit direction (most of them miss)
    E  5 %  origin uniform in the ball of radius 3, zero direction: a ray that stands still
The scenes are geometry_cases.cases."""
import numpy as np

N = 2048
CLASSES = "ABCDE"
SHARES = (0.50, 0.15, 0.15, 0.15, 0.05)
SCALES = (0.25, 0.5, 2.0, 3.7)


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
