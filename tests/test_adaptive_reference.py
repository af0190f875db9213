"""The model of adaptive anti-aliasing (tests/adaptive_reference.py) and the inputs the GPU tests choose, held to the
oracle alone, so that no GPU test can pass vacuously: every scene has edge pixels, supersampling changes edge pixels
(and, with silhouette-only thresholds, pixels the mask leaves alone as well -- a frame that supersampled everything
would be noticed), the border rows and columns hold edge pixels, and the degenerate masks are what they are meant to be.
CPU only.  The scenes are tests/geometry_cases.py at 74 x 45."""
import numpy as np
import pytest

import aa_reference as AA
import adaptive_reference as AR
from geometry_cases import PIPELINES, cases
from helpers import oracle_frame

W, H = 74, 45

_GEOM = {}


def _geom(oracle, kifs, name, distance=None):
    if (name, distance) not in _GEOM:
        screen, cam, gui, iters = _case(kifs, name, distance)
        _GEOM[(name, distance)] = AR.geometry(oracle, kifs, screen, cam, gui, iters)
    return _GEOM[(name, distance)]


def _case(kifs, name, distance=None):
    screen, cam, gui, iters = cases(kifs, W, H)[name]
    if distance is not None:
        cam = kifs.CameraData(origin_distance=distance, phi=cam.phi, theta=cam.theta)
    return screen, cam, gui, iters


# pipeline: edge pixels with silhouette-only thresholds
SILHOUETTE_EDGES = {"julia_24": 99, "julia_25": 128, "genjulia": 163, "sphere": 72, "cylinder": 164, "box": 122, "torus": 120,
                    "sierpinski": 204, "bunny": 79, "unknown_id": 0}
# pipeline: edge pixels with the default thresholds
DEFAULT_EDGES = {"julia_24": 257, "julia_25": 368, "genjulia": 164, "sphere": 108, "cylinder": 260, "box": 299, "torus": 168,
                 "sierpinski": 230, "bunny": 106, "unknown_id": 0}


@pytest.mark.parametrize("name", PIPELINES)
def test_edge_counts_of_the_chosen_scenes(name, oracle, kifs):
    g = _geom(oracle, kifs, name)
    assert int(AR.edge_mask(g, *AR.SILHOUETTE).sum()) == SILHOUETTE_EDGES[name]
    assert int(AR.edge_mask(g, *AR.DEFAULT).sum()) == DEFAULT_EDGES[name]
    if name == "unknown_id":  # every pixel misses: the empty-queue case
        assert (g.view(np.uint32) == np.array([0, 0, 0, AR.MISS_T], dtype=np.uint32)).all()


@pytest.mark.parametrize("name", [n for n in PIPELINES if n != "unknown_id"])
@pytest.mark.parametrize("k", [2, 3])
def test_supersampling_changes_edge_pixels_and_others(name, k, oracle, kifs):
    screen, cam, gui, iters = _case(kifs, name)
    mask = AR.edge_mask(_geom(oracle, kifs, name), *AR.SILHOUETTE)
    plain = oracle_frame(oracle, kifs, screen, cam, gui, iters)
    full = AA.aa_frame(oracle, kifs, screen, cam, gui, iters, k)
    differs = (full != plain).any(-1)
    assert int((differs & mask).sum()) > 0
    if name == "box":  # flat faces: a second sample changes nothing off the silhouette; the edge count carries that side
        assert int((differs & ~mask).sum()) == 0
    else:
        assert int((differs & ~mask).sum()) > 0
    # the model's frame is the plain one off the mask and the supersampled one on it
    want, m2 = AR.expected_frame(oracle, kifs, screen, cam, gui, iters, k, *AR.SILHOUETTE, geom=_geom(oracle, kifs, name))
    assert (m2 == mask).all()
    assert (want[~mask] == plain[~mask]).all() and (want[mask] == full[mask]).all()


def test_border_rows_and_columns_hold_edge_pixels(oracle, kifs):
    e = AR.edge_mask(_geom(oracle, kifs, "sierpinski", 1.1), *AR.DEFAULT)
    assert (int(e[0].sum()), int(e[-1].sum()), int(e[:, 0].sum()), int(e[:, -1].sum())) == (46, 3, 27, 43)


def test_nearly_all_edges(oracle, kifs):
    e = AR.edge_mask(_geom(oracle, kifs, "julia_24", 1.1), *AR.DEFAULT)
    assert int(e.sum()) == 2596 and e.size == 3330


def test_camera_inside_the_box_no_edges(oracle, kifs):
    g = _geom(oracle, kifs, "box", 1.3)
    assert (g[..., 3] == 0).all()  # every pixel hits at t = 0
    assert not AR.edge_mask(g, *AR.DEFAULT).any()


@pytest.mark.parametrize("name", PIPELINES)
def test_all_hits_thresholds_mark_every_hit(name, oracle, kifs):
    g = _geom(oracle, kifs, name)
    hit = g[..., 3].view(np.uint32) != AR.MISS_T
    e = AR.edge_mask(g, *AR.ALL_HITS)
    assert (e[hit]).all()
    assert (e == (hit | AR.edge_mask(g, *AR.SILHOUETTE))).all()


@pytest.mark.parametrize("name", ["julia_25", "torus", "sierpinski"])
def test_mask_is_symmetric(name, oracle, kifs):
    g = _geom(oracle, kifs, name)
    for th in (AR.DEFAULT, AR.SILHOUETTE):
        e = AR.edge_mask(g, *th)
        assert (AR.edge_mask(g.transpose(1, 0, 2), *th) == e.T).all()
        assert (AR.edge_mask(g[::-1], *th) == e[::-1]).all()
        assert (AR.edge_mask(g[:, ::-1], *th) == e[:, ::-1]).all()


def test_pair_rule_on_chosen_texels():
    inf = np.float32(np.inf)
    miss = [0, 0, 0, inf]
    def mask(a, b, nc, dr):
        return AR.edge_mask(np.array([[a, b]], dtype=np.float32), nc, dr).tolist()[0]
    assert mask(miss, miss, 0.9, 0.05) == [False, False]
    assert mask([0, 0, 1, 2.0], miss, -2.0, inf) == [True, True]            # hit against miss, whatever the thresholds
    assert mask([0, 0, 1, 2.0], [0, 0, 1, 2.0], 1.0, 0.0) == [False, False]  # d >= normal_cos and |dt| > 0 both fail
    assert mask([0, 0, 1, 2.0], [0, 1, 0, 2.0], 0.5, 1.0) == [True, True]    # normals apart
    assert mask([0, 0, 1, 2.0], [0, 0, 1, 2.2], 0.5, 0.05) == [True, True]   # 0.2 > 0.05 * 2
    assert mask([0, 0, 1, 2.0], [0, 0, 1, 2.05], 0.5, 0.05) == [False, False]
    nan = np.float32(np.nan)
    assert mask([nan, 0, 1, 2.0], [0, 0, 1, 2.0], -2.0, inf) == [True, True]  # a NaN normal: !(d >= c)
    assert mask([0, 0, 1, 0.0], [0, 0, 1, 0.0], 0.9, inf) == [False, False]   # inf * 0 is NaN: not greater
    one = AR.edge_mask(np.array([[[0, 0, 1, 2.0]]], dtype=np.float32), 2.0, 0.0)  # no neighbour inside the frame
    assert one.tolist() == [[False]]
