"""What a seeded walk (tests/context_walk.py) must cover before the GPU test replays it: every kind of operation at
least twice, at least three tile-table evictions, and at least one return to a geometry the walk has evicted; no
geometry, adaptive or animated launch while supersampling is on (the API refuses them); an adaptive call and an animated
launch on a caller's stream; and a batch beyond 64 views and an animated launch beyond 64 views exactly four view-ring
users apart, so that a slot of the four-deep view-table ring passes from one entry point to the other.  A seed that falls
short is replaced in context_walk.SEEDS; the condition stays."""
import pytest

import context_walk as W


@pytest.mark.parametrize("seed", W.SEEDS)
def test_walk_covers_the_context_state(seed):
    ops = W.plan(seed)
    assert ops == W.plan(seed) and len(ops) == W.STEPS  # a pure function of the seed
    cov = W.coverage(ops)
    assert all(n >= 2 for n in cov["kinds"].values()), cov["kinds"]
    assert cov["evictions"] >= 3 and cov["returns"] >= 1, cov
    assert not any(kind == "geometry" and ss > 1 for kind, ss in _supersampling_at(ops))
    assert not any(kind in ("adaptive", "animation3", "animation66") and ss > 1 for kind, ss in _supersampling_at(ops))
    caller = cov["on_caller_stream"]
    assert caller["adaptive"] >= 1, caller
    assert caller["animation3"] + caller["animation66"] >= 1, caller
    assert cov["view_ring_shared"], [(i, kind) for i, (kind, _) in enumerate(ops) if kind in W.VIEW_RING_USERS]


def _supersampling_at(ops):
    ss = 1
    for kind, arg in ops:
        if kind == "supersampling":
            ss = arg
        yield kind, ss


def test_seeds_differ():
    assert len({tuple(W.plan(s)) for s in W.SEEDS}) == len(W.SEEDS) == 3


def test_model_of_the_table_cache():
    """Nine geometries on eight slots: the first is evicted by the ninth, and coming back to it is a return."""
    ops = [("band", i) for i in range(9)] + [("band", 0), ("band", 8), ("band", 1)]
    events = [e for _, _, e in W.replay(ops)]
    assert events == ["fill"] * 8 + ["evict", "return", "hit", "return"]
    # an animated band lands in the slot of the plain band of its rows; whole frames share the full frame's
    events = [e for _, _, e in W.replay([("band", 7), ("animation3", 7), ("animation3", -1), ("adaptive", 2), ("animation66", 0)])]
    assert events == ["fill", "hit", "fill", "hit", "hit"]


def test_coverage_counts_caller_streams_and_the_shared_view_ring():
    """The two measures the walks are held to, on plans whose answers are plain."""
    ops = [("adaptive", 2), ("stream", 1), ("adaptive", 3), ("animation3", -1), ("stream", 0), ("animation66", 0), ("stream", 2),
           ("animation66", 0)]
    cov = W.coverage(ops)
    assert cov["on_caller_stream"] == {"adaptive": 1, "animation3": 1, "animation66": 1}
    assert not cov["view_ring_shared"]
    A, B = ("animation66", 0), ("batch66", 0)
    assert W.coverage([A, B, B, B, B])["view_ring_shared"]          # the fifth user takes the first one's slot
    assert W.coverage([B, B, B, B, B, A, B, B, B, B])["view_ring_shared"]
    assert not W.coverage([B] * 5)["view_ring_shared"] and not W.coverage([A] * 5 + [("band", 0)])["view_ring_shared"]
    assert not W.coverage([A, B, A, B])["view_ring_shared"]         # both kinds, and the ring never comes round
    assert not W.coverage([A, B, B, A])["view_ring_shared"]
    assert not W.coverage([A, A, B, B, A, A, B, B, A])["view_ring_shared"]  # both in every window, every slot stays with its kind
    assert not W.coverage([A, B, A, B, A, B, A, B])["view_ring_shared"]
