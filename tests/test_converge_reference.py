"""The model of converging accumulation (tests/converge_reference.py) held to the models it must agree with, on the CPU,
so that tests/test_gpu_converge.py cannot pass vacuously: against progressive_reference.fold for identity (b) and
jitter_reference.jittered_frames for identity (a), bit for bit; identity (c); a count near 2^24 freezes a pixel; and the
cases of tests/converge_cases.py say something, shown from the oracle alone, for every pipeline that hits anything."""
import numpy as np
import pytest

import converge_cases as CC
import converge_reference as CR
import jitter_reference as JR
import progressive_reference as PR

F = np.float32
_LIN = {}


def lin_of(oracle, kifs, name):
    if name not in _LIN:
        screen, cam, gui, iters, cams, cells = CC.views(kifs, name)
        _LIN[name] = (JR.linear_views(oracle, kifs, screen, cams, gui, iters, CC.GRID, cells, CC.SAMPLES), screen, gui, iters, cams, cells)
        _LIN[name][0].setflags(write=False)
    return _LIN[name]


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def test_the_rule_as_the_header_words_it():
    sums = np.zeros((1, 1, 6, 4), dtype=F)
    q = np.zeros((1, 1, 6), dtype=F)
    # n = 4 samples of luminance 0.5 each (grey 0.5): L = 2, q = 1, d = 4 - 4 = 0 <= b: settled from min_samples on
    sums[0, 0, 0] = (2.0, 2.0, 2.0, 4.0)
    q[0, 0, 0] = 4 * F(CR.luminance(np.array([0.5, 0.5, 0.5], dtype=F))) ** 2
    # two samples, 0 and 1: d = n q - L^2 = 2 - 1 = 1, b = tol^2 * 4 * 1
    sums[0, 0, 1] = (1.0, 1.0, 1.0, 2.0)
    q[0, 0, 1] = 1.0
    sums[0, 0, 2] = (np.nan, 1.0, 1.0, 4.0)          # a NaN compares false: not settled
    q[0, 0, 2] = 1.0
    sums[0, 0, 3] = (2.0, 2.0, 2.0, 16777214.0)      # settled or not, n + 4 would leave 2^24
    sums[0, 0, 4] = (2.0, 2.0, 2.0, 16777212.0)      # n + 4 == 2^24: allowed
    q[0, 0, 3] = q[0, 0, 4] = 1.0e30                # far from settled
    sums[0, 0, 5] = (1.0, 1.0, 1.0, 2.0)             # as pixel 1 ...
    q[0, 0, 5] = 1.0
    got = CR.active(sums, q, (0.51, 2), 4)[0, 0]
    # pixel 0: d rounds to about 0 <= b = 0.26 * 16 * 3; pixel 1: d = about 1 <= b = 0.2601 * 4 * 1: settled
    assert got.tolist() == [False, False, True, False, True, False]
    assert CR.active(sums, q, (0.51, 5), 4)[0, 0].tolist() == [True, True, True, False, True, True]      # min_samples
    assert CR.active(sums, q, (0.49, 2), 4)[0, 0, 1]                                                    # a tighter tolerance
    assert not CR.active(sums, q, (np.inf, 2), 4)[0, 0, :2].any() and CR.active(sums, q, (np.inf, 2), 4)[0, 0, 2]
    assert CR.tol2(0.25) == F(0.0625) and CR.tol2(np.inf) == F(np.inf)
    y = CR.luminance(np.array([0.3, 0.6, 0.9], dtype=F))
    assert y == F(F(F(0.2126) * F(0.3) + F(0.7152) * F(0.6)) + F(0.0722) * F(0.9)) and y.dtype == F


@pytest.mark.parametrize("encode", [1, 0])
def test_identity_a_and_b_against_the_progressive_and_jittered_models(encode, oracle, kifs):
    lin, screen, gui, iters, cams, cells = lin_of(oracle, kifs, "julia_24")
    passes = PR.split_views(lin, 1, CC.SAMPLES, CC.SPLITS)
    # (a) a restart pass: the jittered call's bytes, the resume call's sums
    first = CR.converged(oracle, passes[:1], [(1 / 16, 4)], encode)[0]
    want = JR.jittered_frames(oracle, kifs, screen, cams[:4], gui, iters, 4, CC.GRID, cells[:4], encode, lin=lin[:4])
    assert (first["frames"] == want).all() and first["mask"].all()
    plane, total = PR.fold(None, 0, passes[0])
    assert total == 4 and (_bits(first["sums"]) == _bits(plane)).all()
    # (b) min_samples above every count reached: the same sequence of resume passes, planes and pictures
    got = CR.converged(oracle, passes, [(1 / 16, 13)] * 3, encode)
    frames, plane, total = PR.carried(oracle, passes, encode)
    for p in range(3):
        assert (got[p]["frames"] == frames[p]).all() and got[p]["mask"].all() and got[p]["counts"].tolist() == [CC.W * CC.H]
    assert (_bits(got[-1]["sums"]) == _bits(plane)).all() and total == 12
    # and the moments are what they say: the sum of the squared luminances, in order
    y = CR.luminance(lin)
    q = (y[0] * y[0]).astype(F)
    for s in range(1, 12):
        q = (q + (y[s] * y[s]).astype(F)).astype(F)
    assert (_bits(got[-1]["moments"][0]) == _bits(q)).all()


def test_identity_c_everything_stops_at_min_samples(oracle, kifs):
    lin = lin_of(oracle, kifs, "julia_24")[0]
    passes = PR.split_views(lin, 1, CC.SAMPLES, CC.SPLITS)
    got = CR.converged(oracle, passes, [(np.inf, 8)] * 3)
    assert [int(g["counts"][0]) for g in got] == [CC.W * CC.H, 0, 0]
    assert got[1]["mask"].all() and not got[2]["mask"].any()
    assert (_bits(got[2]["sums"]) == _bits(got[1]["sums"])).all() and (_bits(got[2]["moments"]) == _bits(got[1]["moments"])).all()
    assert (got[2]["sums"][..., 3] == 8.0).all() and (got[2]["frames"] == got[1]["frames"]).all()


def test_a_count_near_2_24_freezes_a_pixel(oracle, kifs):
    lin = lin_of(oracle, kifs, "julia_24")[0]
    passes = PR.split_views(lin, 1, CC.SAMPLES, CC.SPLITS)
    seeded = CR.converged(oracle, passes[:1], [(0.0, 4)])[0]
    sums, moments = seeded["sums"].copy(), seeded["moments"].copy()
    sums[..., 3] = F(16777216.0 - 6.0)
    rule = (0.0, 4)
    one = CR.converged(oracle, passes[1:2], [rule], sums=sums, moments=moments, restart=False)[0]  # + 4: allowed
    assert one["mask"].any() and (one["sums"][..., 3][one["mask"]] == F(16777214.0)).all() and not one["counts"].any()
    two = CR.converged(oracle, passes[2:], [rule], sums=one["sums"], moments=one["moments"], restart=False)[0]  # + 4: past 2^24
    assert not two["mask"].any() and (_bits(two["sums"]) == _bits(one["sums"])).all() and not two["counts"].any()


@pytest.mark.parametrize("name", CC.PIPELINES)
def test_the_cases_say_something(name, oracle, kifs):
    lin = lin_of(oracle, kifs, name)[0]
    passes = PR.split_views(lin, 1, CC.SAMPLES, CC.SPLITS)
    rule = (CC.tolerance(name), CC.MIN_SAMPLES)
    got = CR.converged(oracle, passes, [rule] * 3)
    counts = [int(g["counts"][0]) for g in got]
    after = [CR.active(g["sums"], g["moments"], rule, CC.PER_PASS)[0] for g in got]
    assert [int(a.sum()) for a in after] == counts
    assert (got[1]["mask"][0] == after[0]).all() and (got[2]["mask"][0] == after[1]).all()  # a pass marches what was left
    if CC.TOLERANCE[name] is None:  # nothing is hit: nothing can stay active
        assert counts == [0, 0, 0]
        return
    assert counts[2] > 0, counts                                    # pixels still active after the last pass
    assert (after[0] & ~after[2]).any()                             # active after pass 1, settled later
    bg = lin[0, 0, 0]
    hit = (lin[:CC.PER_PASS] != bg).any(-1).any(0)
    assert (hit & ~after[0]).any()                                  # hit pixels that settle after pass 1
    none, part, full = CR.blocks(after[2])
    assert none + part + full == 60 and none > 0 and part > 0, (none, part, full)
    settled = ~after[0]                                             # an inactive pixel keeps its bits through pass 2
    assert (_bits(got[1]["sums"])[0][settled] == _bits(got[0]["sums"])[0][settled]).all()
    assert (got[1]["sums"][0][..., 3][after[0]] == 8.0).all() and (got[1]["sums"][0][..., 3][settled] == 4.0).all()


def test_julia_24_is_done_after_two_passes_at_one_eighth(oracle, kifs):
    name, tol = CC.DONE_EARLY
    lin = lin_of(oracle, kifs, name)[0]
    got = CR.converged(oracle, PR.split_views(lin, 1, CC.SAMPLES, CC.SPLITS), [(tol, CC.MIN_SAMPLES)] * 3)
    counts = [int(g["counts"][0]) for g in got]
    assert counts[0] > 0 and counts[1:] == [0, 0] and not got[2]["mask"].any()


def test_a_tightened_tolerance_wakes_settled_pixels(oracle, kifs):
    lin = lin_of(oracle, kifs, "julia_24")[0]
    passes = PR.split_views(lin, 1, CC.SAMPLES, CC.SPLITS)
    loose = CR.converged(oracle, passes, [(1 / 8, 4)] * 3)
    tight = CR.converged(oracle, passes, [(1 / 8, 4), (1 / 64, 4), (1 / 64, 4)])
    assert tight[1]["mask"].sum() > loose[1]["mask"].sum() and (tight[1]["mask"] | ~loose[1]["mask"]).all()
