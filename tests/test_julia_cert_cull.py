"""The certified cull radius of the power-2 Julia set (julia_cull_radius, fill_params, fill_views in kifs_schedule.cpp;
DESIGN section 4), on the CPU through the C ABI's host model:

  * the bound D(rho) the certificate promises holds against the NumPy oracle's estimate at every sampled point of the
    shell rho <= |p| <= 2 + epsilon, and stays above epsilon;
  * the function refuses what it must, and the thresholds are then today's, bit for bit;
  * a view beyond |origin|^2 = 1024 sends the whole launch back to the patch sphere;
  * a NumPy replay of the headline frame finds no hit among the rays the new cull removes, and the cull removes at
    least 40 % of the rays the patch sphere's cull marches.
"""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest

F = np.float32
HEADLINE_C = (-0.2, 0.6, 0.2, 0.2)
REFERENCE_C = (-0.1, 0.6, 0.9, -0.3)
SMALL_C = (0.05, 0.0, 0.0, 0.0)
MAX_DISTANCE = 1000.0


def _random_constants():
    rng = np.random.default_rng(20261019)
    out = []
    for norm in rng.uniform(0.2, 1.2, size=3):
        v = rng.normal(size=4)
        out.append(tuple(float(x) for x in F(v / np.linalg.norm(v) * norm)))
    return out


CONSTANTS = [HEADLINE_C, REFERENCE_C, SMALL_C] + _random_constants()


def radius(kifs, c, epsilon, max_distance, sdf_iters):
    """(rho, D(rho)) of the C ABI; rho == 0.0: no certificate."""
    from kifs_raymarching_amd._lib import lib
    bound = C.c_double(-1.0)
    rho = lib.kifs_host_julia_cull_radius((C.c_float * 4)(*c), epsilon, max_distance, sdf_iters, C.byref(bound))
    return rho, bound.value


def thresholds(kifs, screen, options, sdf_iters, cameras):
    """(cull_n2, quick_cull_n2, tile_cull_sqrtk, tile_cull_beta, shape_n2) of a launch, as float32."""
    from kifs_raymarching_amd._lib import lib
    cams = kifs.camera_array(cameras)
    out = (C.c_float * 5)()
    s = screen.into_buffer_data()
    assert lib.kifs_host_cull_thresholds(C.byref(s), C.byref(options), sdf_iters, cams, len(cameras), out) == 0
    return tuple(F(v) for v in out)


def patch_sphere(epsilon, height, B=2.0, quick=True):
    """Today's thresholds, in the float32 operations fill_params uses."""
    R = F(B) + F(epsilon)
    cull, q = F(1.1) * R * R, (F(1.2) * R * R if quick else F(0.0))
    beta = F(34.0) / F(height) if (quick and height >= 64) else F(0.0)
    return cull, q, np.sqrt(q), beta, cull


def certified(rho, height):
    r = F(rho)
    cull = (F(1.0) + F(2.0 ** -6)) * r * r
    q = cull * (F(1.2) / F(1.1))
    return cull, q, np.sqrt(q), (F(34.0) / F(height) if height >= 64 else F(0.0))


def julia_options(kifs, c, epsilon=1e-4, max_distance=MAX_DISTANCE, group=1, heatmap=False, prim=0):
    return kifs.GuiData(max_iterations=256, max_distance=max_distance, epsilon=epsilon, is_heatmap=heatmap,
                        fractal_group=kifs.FractalGroup(group), primitive_shape=kifs.PrimitiveShape(prim),
                        constant=c).into_buffer_data()


# ---- the bound against the oracle ----------------------------------------------------------------------------------
def _shell_points(rng, lo, hi, n_shell, n_edge):
    d = rng.normal(size=(3, n_shell + n_edge))
    d /= np.linalg.norm(d, axis=0)
    r = np.concatenate([rng.uniform(lo, hi, size=n_shell), np.full(n_edge, lo)])
    return [F(d[k] * r) for k in range(3)]


@pytest.mark.parametrize("epsilon", [1e-4, 1e-2])
@pytest.mark.parametrize("index", range(len(CONSTANTS)))
def test_the_bound_holds_against_the_oracle(kifs, index, epsilon):
    from oracle import kifs_oracle_np as NP
    c = CONSTANTS[index]
    rng = np.random.default_rng(1000 * index + int(epsilon * 1e4))
    certificates = 0
    for sdf_iters in (0, 1, 2, 12, 100):
        rho, D = radius(kifs, c, epsilon, MAX_DISTANCE, sdf_iters)
        if index < 3:
            assert rho > 0.0, (c, epsilon, sdf_iters)
        if rho == 0.0:
            continue
        certificates += 1
        eps32 = F(epsilon)
        assert D >= 16.0 * float(eps32) + 2.0 ** -14 and rho <= 2.0 + float(eps32)
        # inside the patch sphere by a float32 rounding, so that every sample takes the orbit's branch of the estimate
        top = (2.0 + float(eps32)) * (1.0 - 2.0 ** -20)
        p = _shell_points(rng, rho, top, 100_000, 10_000)
        s = SimpleNamespace(epsilon=eps32, sdf_iters=sdf_iters, max_distance=F(MAX_DISTANCE), c=[F(x) for x in c])
        d = NP.julia_sdf(s, p).astype(np.float64)
        print(f"c={c} eps={epsilon} iters={sdf_iters}: rho={rho:.6f} D={D:.6f} min d={d.min():.6f}")
        assert np.isfinite(d).all()
        assert d.min() >= D * (1.0 - 1e-3), (c, epsilon, sdf_iters, rho, D, d.min())
        assert (d > float(eps32)).all()
    assert certificates >= (5 if index < 3 else 0)


def test_the_issue_s_figures(kifs):
    """D(1.48) = 0.0029, D(1.50) = 0.0104, D(1.60) = 0.067 for the headline constant; D(1.7) = 0.0083 and D(1.8) = 0.064
    for the reference constant -- through the radius: the bisection lands where D = 16 epsilon + 2^-14."""
    def D(c, rho, iters):
        cn = math.sqrt(sum(float(F(x)) ** 2 for x in c))
        a = math.sqrt(rho * rho + 0.01)
        L, P = a, 1.0
        for _ in range(iters):
            if L > 1e150:
                break
            P *= 1.0 - cn / (L * L)
            L = L * L - cn
        return 0.5 * a * (math.log(a * a - cn) - math.log(a)) * P
    assert abs(D(HEADLINE_C, 1.48, 12) - 0.0029) < 2e-4 and abs(D(HEADLINE_C, 1.50, 12) - 0.0104) < 2e-4
    assert abs(D(HEADLINE_C, 1.60, 12) - 0.067) < 1e-3
    assert abs(D(REFERENCE_C, 1.7, 100) - 0.0083) < 2e-4 and abs(D(REFERENCE_C, 1.8, 100) - 0.064) < 1e-3
    for c, iters in ((HEADLINE_C, 12), (REFERENCE_C, 100), (SMALL_C, 12)):
        for eps in (1e-4, 1e-2):
            rho, bound = radius(kifs, c, eps, MAX_DISTANCE, iters)
            need = 16.0 * float(F(eps)) + 2.0 ** -14
            assert abs(D(c, rho, iters) - bound) <= 1e-12 and need <= bound
            if c != SMALL_C:  # (its radius is set by the float32 range of dqs: slow trips just beyond the escape radius)
                # (the bisection stops at 2^-36 of the shell and dD/drho < 1 there: 1e-11 over, against need >= 2^-14)
                assert bound <= need * (1.0 + 1e-6)
            bigger, _ = radius(kifs, c, eps, MAX_DISTANCE, iters + 1 if iters < 100 else iters)
            assert bigger >= rho  # more trips, a smaller product: never a smaller radius
    assert 1.47 < radius(kifs, HEADLINE_C, 1e-4, MAX_DISTANCE, 12)[0] < 1.48
    assert 1.67 < radius(kifs, REFERENCE_C, 1e-4, MAX_DISTANCE, 100)[0] < 1.70


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_keep_today_s_thresholds(kifs):
    H = 144
    screen = kifs.ScreenData(256, H)
    cam = [kifs.CameraData(origin_distance=5.0)]
    assert radius(kifs, (3.0, 0.0, 0.0, 0.0), 1e-4, MAX_DISTANCE, 12) == (0.0, 0.0)
    assert radius(kifs, (float("nan"), 0.6, 0.2, 0.2), 1e-4, MAX_DISTANCE, 12) == (0.0, 0.0)
    assert radius(kifs, HEADLINE_C, 1e-4, 1e14, 100) == (0.0, 0.0)     # dqs could leave float32
    assert radius(kifs, HEADLINE_C, 1.0, MAX_DISTANCE, 12) == (0.0, 0.0)  # 16 epsilon is beyond the shell
    assert radius(kifs, HEADLINE_C, -1e-4, MAX_DISTANCE, 12) == (0.0, 0.0)
    assert radius(kifs, HEADLINE_C, 1e-4, 1e15, 12) == (0.0, 0.0)
    assert radius(kifs, (2000.0, 0.0, 0.0, 0.0), 1e-4, MAX_DISTANCE, 12) == (0.0, 0.0)
    # the thresholds of launches without a certificate: the patch sphere's, bit for bit
    for c, eps, md, iters in (((3.0, 0.0, 0.0, 0.0), 1e-4, MAX_DISTANCE, 12), (HEADLINE_C, 1e-4, 1e14, 100),
                              (HEADLINE_C, 1.0, MAX_DISTANCE, 12)):
        got = thresholds(kifs, screen, julia_options(kifs, c, eps, md), iters, cam)
        assert got == patch_sphere(eps, H), (c, eps, md)
    nan = julia_options(kifs, HEADLINE_C)
    nan.constant[0] = float("nan")
    assert thresholds(kifs, screen, nan, 12, cam) == patch_sphere(1e-4, H)
    # heatmap frames march every ray: cull_n2 as ever, the quick exits off
    assert thresholds(kifs, screen, julia_options(kifs, HEADLINE_C, heatmap=True), 12, cam) == patch_sphere(1e-4, H, quick=False)
    # other pipelines: the generalised Julia set (same patch, no certificate yet), a KIFS sphere
    assert thresholds(kifs, screen, julia_options(kifs, HEADLINE_C, group=2), 12, cam) == patch_sphere(1e-4, H)
    assert thresholds(kifs, screen, julia_options(kifs, HEADLINE_C, group=0), 12, cam) == patch_sphere(1e-4, H, B=1.0)
    # and with a certificate: (1 + 2^-6) rho^2, the quick exits in their ratio, the shape rules' sphere unmoved
    for c, eps, iters in ((HEADLINE_C, 1e-4, 12), (REFERENCE_C, 1e-4, 100), (SMALL_C, 1e-2, 12)):
        rho, _ = radius(kifs, c, eps, MAX_DISTANCE, iters)
        got = thresholds(kifs, screen, julia_options(kifs, c, eps), iters, cam)
        assert got[:4] == certified(rho, H) and got[4] == patch_sphere(eps, H)[4]
        assert got[0] < got[4]
    small = thresholds(kifs, kifs.ScreenData(96, 48), julia_options(kifs, HEADLINE_C), 12, cam)
    assert small[3] == 0.0 and small[:3] == certified(radius(kifs, HEADLINE_C, 1e-4, MAX_DISTANCE, 12)[0], 48)[:3]


# ---- views ------------------------------------------------------------------------------------------------------------
def test_a_distant_view_sends_the_launch_back_to_the_patch_sphere(kifs):
    H = 144
    screen = kifs.ScreenData(256, H)
    opts = julia_options(kifs, HEADLINE_C)
    rho, _ = radius(kifs, HEADLINE_C, 1e-4, MAX_DISTANCE, 12)
    near = [kifs.CameraData(origin_distance=d, phi=0.3 * d) for d in (5.0, 2.05, 31.9)]
    assert thresholds(kifs, screen, opts, 12, near)[:4] == certified(rho, H)
    for far in (32.1, 500.0):
        views = near[:2] + [kifs.CameraData(origin_distance=far)]
        assert thresholds(kifs, screen, opts, 12, views) == patch_sphere(1e-4, H)
        assert thresholds(kifs, screen, opts, 12, views[::-1]) == patch_sphere(1e-4, H)
    # a matrix that is not orthonormal switches the tile-level exit off and nothing else, with or without a distant view
    skew = near[0].into_buffer_data()
    skew.matrix[1][0] = skew.matrix[1][0] * 1.5 + 0.25
    got = thresholds(kifs, screen, opts, 12, [near[1], skew])
    assert got[:3] == certified(rho, H)[:3] and got[3] == 0.0
    got = thresholds(kifs, screen, opts, 12, [skew, kifs.CameraData(origin_distance=40.0)])
    assert got[:3] == patch_sphere(1e-4, H)[:3] and got[3] == 0.0 and got[4] == patch_sphere(1e-4, H)[4]
    # an origin beyond 1e15: no culls at all, as before
    gone = near[0].into_buffer_data()
    gone.origin[0] = 3.0e15
    got = thresholds(kifs, screen, opts, 12, [near[0], gone])
    assert got[0] == 0.0 and got[1] == 0.0 and got[3] == 0.0 and got[4] == 0.0


# ---- replay -----------------------------------------------------------------------------------------------------------
def test_replay_of_the_headline_frame(kifs, oracle):
    """480 x 270 of the headline workload at distance 5, marched by the NumPy oracle without any cull: no ray whose closest
    approach to the origin exceeds the cull's radius hits, and the cull takes at least 40 % of the rays that the patch
    sphere's cull marches (0.54 at 1080p)."""
    from kifs_raymarching_amd.configs import WORKLOADS
    from oracle import kifs_oracle_np as NP
    from helpers import oracle_uniforms
    w = WORKLOADS["cfg2_julia_1080p"]
    screen = kifs.ScreenData(480, 270)
    s, c, o = oracle_uniforms(oracle, kifs, (screen, w.camera, w.gui))
    it = oracle.iters(*w.iters)
    _, _, hit = NP.render_linear(s, c, o, it)
    opts = w.gui.into_buffer_data()
    rho, _ = radius(kifs, tuple(opts.constant), opts.epsilon, opts.max_distance, w.iters[0])
    cull_n2, _, _, _, old_n2 = (float(v) for v in thresholds(kifs, screen, opts, w.iters[0], [w.camera]))
    assert rho > 0.0 and cull_n2 == float(certified(rho, 270)[0])
    # closest approaches of the frame's rays, in double
    sc = NP.Scene(s, c, o, it)
    ys, xs = np.mgrid[0:270, 0:480]
    uvx = 2.0 * (xs + 0.5) / 270.0 - float(sc.aspect)
    uvy = 2.0 * (ys + 0.5) / 270.0 - 1.0
    m = np.array(sc.m, dtype=np.float64)
    d = np.stack([uvx * m[1][k] - uvy * m[2][k] - m[0][k] for k in range(3)], axis=-1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    org = np.array(sc.origin, dtype=np.float64)
    b = -(d @ org)
    c2 = np.where(b <= 0.0, org @ org, org @ org - b * b)
    marched_today = c2 <= old_n2
    culled_now = c2 > cull_n2
    share = (marched_today & culled_now).sum() / marched_today.sum()
    print(f"rho = {rho:.4f}: {marched_today.sum()} rays marched today, {share:.3f} of them culled, {hit.sum()} hits")
    assert hit.sum() > 1000
    assert not (hit & (c2 > rho * rho)).any()
    assert share >= 0.4
