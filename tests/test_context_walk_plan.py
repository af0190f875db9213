"""What a seeded walk (tests/context_walk.py) must cover before the GPU test replays it: every kind of operation at
least twice, at least three tile-table evictions, and at least one return to a geometry the walk has evicted.  A seed
that falls short is replaced in context_walk.SEEDS; the condition stays."""
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
