"""tests/ray_reference.c IS the oracle's march for a ray record, and tests/ray_cases.py gives it something to say: what
makes the GPU comparisons of tests/test_gpu_rays.py mean something.  CPU only.
  * For the pixel rays of a frame of every pipeline the reference's texels are geometry_reference.march's bit for bit
    and its colours kor_render's bytes, both encodes, and again with heatmap on.
  * For the generated rays, from the reference alone: enough hits, enough misses, hits in the classes with interior
    origins and scaled directions, no NaN.
  * configs.pixel_rays is kor_ray_direction bit for bit."""
import ctypes as C

import numpy as np
import pytest

import geometry_reference as GR
import ray_cases
import ray_reference as RR
from geometry_cases import PIPELINES, cases
from helpers import oracle_uniforms

W, H = 64, 48


def oracle_pixel_rays(O, s, c):
    """(H * W, 8) float32: the camera's origin and kor_ray_direction of every pixel, row by row."""
    w, h = int(s.width), int(s.height)
    rays = np.zeros((h * w, 8), dtype=np.float32)
    rays[:, 0:3] = np.array(c.origin[:], dtype=np.float32)
    d = (C.c_float * 3)()
    fn = O.lib().kor_ray_direction
    for y in range(h):
        for x in range(w):
            fn(C.byref(s), C.byref(c), x, y, d)
            rays[y * w + x, 4:7] = d[:]
    return rays


@pytest.mark.parametrize("name", PIPELINES)
def test_the_restatement_is_the_oracles_march(name, kifs, oracle):
    screen, cam, gui, iters = cases(kifs, W, H)[name]
    s, c, o = oracle_uniforms(oracle, kifs, (screen, cam, gui))
    it = oracle.iters(*iters)
    rays = oracle_pixel_rays(oracle, s, c)
    want_geom, want_hit, want_steps = GR.march(oracle, s, c, o, it)
    for heatmap in (0, 1):
        o.is_heatmap = heatmap
        for encode in (0, 1):
            geom, rgba, steps = RR.trace(oracle, o, it, rays, encode)
            assert (geom.view(np.uint32) == want_geom.reshape(-1, 4).view(np.uint32)).all()
            assert (steps == want_steps.reshape(-1)).all()
            assert (RR.hits(geom) == want_hit.reshape(-1)).all()
            want = oracle.render(s, c, o, it, encode=encode)
            assert (rgba == want.reshape(-1, 4)).all(), (heatmap, encode, int((rgba != want.reshape(-1, 4)).any(-1).sum()))


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("name", [p for p in PIPELINES if p != "unknown_id"])
def test_the_generated_rays_hit_and_miss_in_every_class(name, seed, kifs, oracle):
    _, _, gui, iters = cases(kifs, W, H)[name]
    rays, labels = ray_cases.rays(seed)
    assert rays.shape == (ray_cases.N, 8) and rays.dtype == np.float32
    geom, _, _ = RR.trace_scene(oracle, kifs, gui, iters, rays)
    hit = RR.hits(geom)
    per_class = {c: int(hit[labels == c].sum()) for c in ray_cases.CLASSES}
    print(f"{name} seed {seed}: {int(hit.sum())} hits of {hit.size}, per class {per_class}")
    assert hit.sum() >= 0.10 * hit.size and (~hit).sum() >= 0.10 * hit.size, (int(hit.sum()), per_class)
    for c in "ABC":
        assert per_class[c] >= 10, per_class
    assert not np.isnan(geom).any()
    assert (geom[~hit].view(np.uint32) == RR.MISS).all()


def test_the_generator_is_seeded_and_keeps_its_classes():
    a, la = ray_cases.rays(1)
    b, lb = ray_cases.rays(1)
    c, _ = ray_cases.rays(2)
    assert (a.view(np.uint32) == b.view(np.uint32)).all() and (la == lb).all() and (a != c).any()
    counts = {k: int((la == k).sum()) for k in ray_cases.CLASSES}
    assert counts == {"A": 1024, "B": 307, "C": 307, "D": 307, "E": 103}, counts
    d = a[:, 4:7].astype(np.float64)
    length = np.linalg.norm(d, axis=1)
    assert (length[la == "E"] == 0).all()
    assert np.allclose(length[(la == "A") | (la == "C") | (la == "D")], 1.0, atol=1e-6)
    assert set(np.round(length[la == "B"], 2)) == {0.25, 0.5, 2.0, 3.7}
    assert (np.linalg.norm(a[la == "C", 0:3], axis=1) <= 1.2 + 1e-6).all()
    assert (a[:, 3] == 0).all() and (a[:, 7] == 0).all()


@pytest.mark.parametrize("name", [p for p in PIPELINES if p != "unknown_id"])
def test_the_grazing_rays_hit_and_miss_at_every_distance(name, kifs, oracle):
    """ray_cases.grazing, from the reference alone (it has no cull): at every origin distance, on either side of the ray
    kernel's |o|^2 <= 1024 switch, at least 30 rays hit and 30 miss -- a cull that took a hitting ray, or a march that
    lost one from far away, would change bits the GPU comparison looks at."""
    _, _, gui, iters = cases(kifs, W, H)[name]
    rays, dist, length = ray_cases.grazing(3, ray_cases.BOUND[name], ray_cases.N_GRAZING_OF.get(name, ray_cases.N_GRAZING))
    assert rays.shape == (ray_cases.N_GRAZING_OF.get(name, ray_cases.N_GRAZING), 8) and rays.dtype == np.float32
    geom, _, _ = RR.trace_scene(oracle, kifs, gui, iters, rays)
    hit = RR.hits(geom)
    per = {d: (int(hit[dist == d].sum()), int((~hit)[dist == d].sum())) for d in ray_cases.DISTANCES}
    print(f"{name}: hits, misses per distance {per}; hits per length "
          f"{ {l: int(hit[length == l].sum()) for l in ray_cases.LENGTHS} }")
    assert all(h >= 30 and m >= 30 for h, m in per.values()), per
    assert not np.isnan(geom).any()


def test_the_grazing_generator_is_seeded_and_tangent():
    a, da, la = ray_cases.grazing(3, 2.0)
    b, db, lb = ray_cases.grazing(3, 2.0)
    c, _, _ = ray_cases.grazing(4, 2.0)
    assert (a.view(np.uint32) == b.view(np.uint32)).all() and (da == db).all() and (la == lb).all() and (a != c).any()
    o, d = a[:, 0:3].astype(np.float64), a[:, 4:7].astype(np.float64)
    assert np.allclose(np.linalg.norm(o, axis=1), da, rtol=1e-6) and np.allclose(np.linalg.norm(d, axis=1), la, rtol=1e-6)
    for dist in ray_cases.DISTANCES:
        assert {l: int(((da == dist) & (la == l)).sum()) for l in ray_cases.LENGTHS} == {0.5: 200, 1.0: 200}
    oo = (o * o).sum(1)
    assert (oo[da <= 31.9] <= 1024.0).all() and (oo[da == 32.1] > 1024.0).all()  # either side of the cull's switch
    od = (o * d).sum(1)
    assert (od < 0).all()  # every ray approaches
    closest = np.sqrt(oo - od * od / (d * d).sum(1))  # of the ray's line: u * bound
    assert (closest >= 0.3 * 2.0 - 1e-3).all() and (closest <= 1.15 * 2.0 + 1e-3).all()
    assert (closest > 2.2).sum() >= 50 and (closest < 1.0).sum() >= 100  # beyond the radius the cull stands on, and well inside
    tall, dt, _ = ray_cases.grazing(3, ray_cases.BOUND["cylinder"])  # the tangent sphere stays short of an origin at 2.5
    o, d = tall[:, 0:3].astype(np.float64), tall[:, 4:7].astype(np.float64)
    closest = np.sqrt((o * o).sum(1) - (o * d).sum(1) ** 2 / (d * d).sum(1))
    assert (closest[dt == 2.5] <= 0.95 * 2.5 + 1e-3).all() and closest[dt == 8.0].max() > 1.1 * ray_cases.BOUND["cylinder"]
    assert (a[:, 3] == 0).all() and (a[:, 7] == 0).all()


def _lens_camera(kifs):
    from kifs_raymarching_amd.configs import lens_cameras
    return lens_cameras(kifs.CameraData(origin_distance=3.0, phi=0.4, theta=0.2), 0.15, 2.5, 4)[3]


@pytest.mark.parametrize("size", [(64, 48), (74, 45), (33, 9)])
def test_pixel_rays_are_the_oracles_directions(size, kifs, oracle):
    from kifs_raymarching_amd.configs import pixel_rays
    screen = kifs.ScreenData(*size)
    cams = [kifs.CameraData(origin_distance=3.0, phi=0.3), kifs.CameraData(origin_distance=2.5, phi=0.7, theta=0.4),
            kifs.CameraData(origin_distance=5.0, phi=2.1, theta=-0.4), _lens_camera(kifs)]
    for cam in cams:
        got = pixel_rays(screen, cam)
        s = oracle.from_bytes(oracle.Screen, kifs.uniform_bytes(screen.into_buffer_data()))
        raw = cam.into_buffer_data() if hasattr(cam, "into_buffer_data") else cam
        c = oracle.from_bytes(oracle.Camera, kifs.uniform_bytes(raw))
        want = oracle_pixel_rays(oracle, s, c)
        assert got.shape == want.shape and got.dtype == np.float32
        assert (got.view(np.uint32) == want.view(np.uint32)).all(), int((got.view(np.uint32) != want.view(np.uint32)).any(-1).sum())


def test_the_lens_camera_of_this_file_is_sheared(kifs):
    m0 = np.array(_lens_camera(kifs).matrix[0][:3], dtype=np.float64)
    assert abs(np.linalg.norm(m0) - 1.0) > 1e-4  # not unit: pixel_rays may not assume an orthonormal matrix


def test_panorama_rays_are_unit_and_cover_the_sphere(kifs):
    from kifs_raymarching_amd.configs import panorama_rays
    r = panorama_rays((0.5, -1.0, 2.0), 16, 8)
    assert r.shape == (128, 8) and r.dtype == np.float32
    assert (r[:, 0:3] == np.array([0.5, -1.0, 2.0], dtype=np.float32)).all()
    d = r[:, 4:7].astype(np.float64)
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-6)
    rows = d.reshape(8, 16, 3)
    assert (np.diff(rows[:, 0, 2]) < 0).all()               # latitude falls from row to row, the same along a row
    assert np.allclose(rows[:, :, 2], rows[:, :1, 2])
    lon = np.arctan2(rows[3, :, 1], rows[3, :, 0])
    # longitude runs -pi .. pi over the columns, through the column centres
    assert np.allclose(lon, 2.0 * np.pi * (np.arange(16) + 0.5) / 16 - np.pi)
