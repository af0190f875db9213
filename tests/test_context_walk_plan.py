"""What a seeded walk (tests/context_walk.py) must cover before the GPU test replays it: every kind of operation at
least twice, at least three tile-table evictions, and at least one return to a geometry the walk has evicted; no
geometry, adaptive or animated launch while supersampling is on (the API refuses them); an adaptive call and an animated
launch on a caller's stream; and a batch beyond 64 views and an animated launch beyond 64 views exactly four view-ring
users apart, so that a slot of the four-deep view-table ring passes from one entry point to the other.  Since the
accumulated launches joined: none of them while supersampling is on either; a blur or pairs launch and a jittered launch
on a caller's stream; a slot of the scene-table ring passing between an animated and an accumulated launch; and a
view-table slot passing between "accumulate66" and one of the two older users, besides the passage between batch and
animation.  Since progressive accumulation joined ("progressive", "progressive_jitter": two passes each, every pass a
user of the scene ring): neither while supersampling is on; at least one of them on a caller's stream; a scene-table slot
passing between a pass and an animated launch, and one passing between a pass and an accumulated launch.  Since
converging accumulation and ray queries joined ("converge": two passes, "settle": three, every pass a user of the scene
ring under the entry point "converge"; "trace": no table and no ring): neither converging kind while supersampling is on
and at least one trace while it is 2; at least one of the converging kinds and at least one trace on a caller's stream; a
scene-table slot passing between a converging pass and an animated launch, and one passing between a converging pass and
an accumulated launch or a progressive pass.  A seed that falls short is replaced in context_walk.SEEDS; the condition
stays."""
import numpy as np
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
    assert not any(kind in W.ACCUMULATED and ss > 1 for kind, ss in _supersampling_at(ops))
    caller = cov["on_caller_stream"]
    assert caller["adaptive"] >= 1, caller
    assert caller["animation3"] + caller["animation66"] >= 1, caller
    assert caller["accumulate"] + caller["accumulate66"] >= 1 and caller["jitter"] >= 1, caller
    view_users = [(i, kind) for i, (kind, _) in enumerate(ops) if kind in W.VIEW_RING_USERS]
    assert cov["view_ring_shared"], view_users
    assert cov["view_ring_passages"] & {frozenset(("accumulate66", "batch66")), frozenset(("accumulate66", "animation66"))}, view_users
    assert cov["scene_ring_shared"], [(i, kind) for i, (kind, _) in enumerate(ops) if kind in W.ANIMATED or kind in W.ACCUMULATED]
    assert not any(kind in W.PROGRESSIVE and ss > 1 for kind, ss in _supersampling_at(ops))
    assert caller["progressive"] + caller["progressive_jitter"] >= 1, caller
    scene_users = [(i, kind) for i, (kind, _) in enumerate(ops) if kind in W.ANIMATED or kind in W.ACCUMULATED or kind in W.PROGRESSIVE]
    assert frozenset(("progressive", "animation")) in cov["scene_ring_passages"], scene_users
    assert frozenset(("progressive", "accumulate")) in cov["scene_ring_passages"], scene_users
    assert not any(kind in W.CONVERGING and ss > 1 for kind, ss in _supersampling_at(ops))
    assert any(kind == "trace" and ss == 2 for kind, ss in _supersampling_at(ops))
    assert caller["converge"] + caller["settle"] >= 1 and caller["trace"] >= 1, caller
    scene_users = [(i, kind) for i, (kind, _) in enumerate(ops) if kind in W.ANIMATED or kind in W.ACCUMULATED or kind in W.PROGRESSIVE
                   or kind in W.CONVERGING]
    assert frozenset(("converge", "animation")) in cov["scene_ring_passages"], scene_users
    assert cov["scene_ring_passages"] & {frozenset(("converge", "accumulate")), frozenset(("converge", "progressive"))}, scene_users


# per seed: what the blur and jitter models of its walk cost, in per-pixel linear views -- the progressive kinds' passes
# are modelled from the views of their one-call twins, so they are counted here too, and so are the eight views of a
# modelled "converge"
LINEAR_VIEWS = {3757: 4, 9353: 4, 19124: 20}


@pytest.mark.parametrize("seed", W.SEEDS)
def test_linear_views_of_a_walk(seed):
    """The distinct linear views a walk's blur and jitter launches are modelled from, counted from the plan: at most four
    per context state for blur and eight for jitter, none beyond MODEL_UP_TO, and the recorded count per seed -- the CPU
    cost of the new references is visible before a GPU run (0.01 s to 0.19 s per view at these sizes)."""
    keys = W.linear_view_keys(W.plan(seed))
    assert len(keys) == LINEAR_VIEWS[seed], len(keys)
    assert all(W.modelled(k[0]) for k in keys)
    states = {}
    for k in keys:
        states.setdefault(k[:1] + k[2:5], set()).add(k)
    assert all(sum(1 for k in v if k[6] is None) <= 4 and sum(1 for k in v if k[6] is not None) <= 8 for v in states.values())


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
    # and so do the accumulated launches: a banded one the plain band's key, a whole-frame one the full frame's
    ops = [("band", 7), ("accumulate", 7), ("band", 5), ("jitter", 5), ("accumulate", 2), ("band", 2), ("accumulate", -1), ("jitter", -1),
           ("accumulate66", 0), ("animation3", -1)]
    assert [e for _, _, e in W.replay(ops)] == ["fill", "hit", "fill", "hit", "fill", "hit", "fill", "hit", "hit", "hit"]
    assert [k for _, k, _ in W.replay([("screen", 2), ("jitter", 5), ("accumulate66", 0)])] == \
        [(64, 40) + W.band_rows(40, 5) + (None,), (64, 40, 0, 40, None)]
    # and the progressive kinds: the key of the band or frame they render (the lone launch between the passes renders it too)
    ops = [("band", 7), ("progressive", 7), ("progressive_jitter", 5), ("band", 5), ("jitter", 5), ("progressive", -1), ("animation3", -1),
           ("progressive_jitter", -1), ("progressive", 2), ("accumulate", 2)]
    assert [e for _, _, e in W.replay(ops)] == ["fill", "hit", "fill", "hit", "hit", "fill", "hit", "hit", "fill", "hit"]
    assert [k for _, k, _ in W.replay([("screen", 2), ("progressive_jitter", 5), ("progressive", -1)])] == \
        [(64, 40) + W.band_rows(40, 5) + (None,), (64, 40, 0, 40, None)]
    # and the converging kinds: "converge" the band's or the frame's key, "settle" the frame's; a trace takes no table at all
    ops = [("band", 7), ("converge", 7), ("trace", 3), ("settle", 0), ("trace", 7), ("converge", -1), ("animation3", -1), ("converge", 2),
           ("band", 2), ("trace", 2)]
    assert [(i, e) for i, _, e in W.replay(ops)] == [(0, "fill"), (1, "hit"), (3, "fill"), (5, "hit"), (6, "hit"), (7, "fill"), (8, "hit")]
    assert [k for _, k, _ in W.replay([("screen", 2), ("converge", 7), ("trace", 1), ("settle", 0)])] == \
        [(64, 40) + W.band_rows(40, 7) + (None,), (64, 40, 0, 40, None)]
    # eight traces between them do not age a slot: nine geometries are needed for the first eviction, as before
    ops = [("band", i) for i in range(8)] + [("trace", i) for i in range(8)] + [("band", 0), ("band", 8)]
    assert [e for _, _, e in W.replay(ops)] == ["fill"] * 8 + ["hit", "evict"]


def test_coverage_counts_caller_streams_and_the_shared_view_ring():
    """The two measures the walks are held to, on plans whose answers are plain."""
    ops = [("adaptive", 2), ("stream", 1), ("adaptive", 3), ("animation3", -1), ("stream", 0), ("animation66", 0), ("stream", 2),
           ("animation66", 0)]
    cov = W.coverage(ops)
    assert cov["on_caller_stream"] == {"adaptive": 1, "animation3": 1, "animation66": 1, "accumulate": 0, "jitter": 0, "accumulate66": 0,
                                       "progressive": 0, "progressive_jitter": 0, "converge": 0, "settle": 0, "trace": 0}
    cov = W.coverage([("jitter", 5), ("stream", 2), ("jitter", -1), ("accumulate66", 0), ("stream", 0), ("accumulate", 2)])
    assert cov["on_caller_stream"] == {"adaptive": 0, "animation3": 0, "animation66": 0, "accumulate": 0, "jitter": 1, "accumulate66": 1,
                                       "progressive": 0, "progressive_jitter": 0, "converge": 0, "settle": 0, "trace": 0}
    assert not cov["view_ring_shared"]
    A, B = ("animation66", 0), ("batch66", 0)
    assert W.coverage([A, B, B, B, B])["view_ring_shared"]          # the fifth user takes the first one's slot
    assert W.coverage([B, B, B, B, B, A, B, B, B, B])["view_ring_shared"]
    assert not W.coverage([B] * 5)["view_ring_shared"] and not W.coverage([A] * 5 + [("band", 0)])["view_ring_shared"]
    assert not W.coverage([A, B, A, B])["view_ring_shared"]         # both kinds, and the ring never comes round
    assert not W.coverage([A, B, B, A])["view_ring_shared"]
    assert not W.coverage([A, A, B, B, A, A, B, B, A])["view_ring_shared"]  # both in every window, every slot stays with its kind
    assert not W.coverage([A, B, A, B, A, B, A, B])["view_ring_shared"]
    # the view ring by pair of kinds: "accumulate66" (P) is a third user
    P = ("accumulate66", 0)
    pair = lambda a, b: frozenset((a[0], b[0]))
    cov = W.coverage([P, B, B, B, B])
    assert cov["view_ring_passages"] == {pair(P, B)} and not cov["view_ring_shared"]  # (shared: batch against animation alone)
    assert W.coverage([B, B, B, B, P])["view_ring_passages"] == {pair(P, B)}
    assert W.coverage([A, P, B, B, P, A, A, B])["view_ring_passages"] == {pair(A, P), pair(A, B)}
    assert W.coverage([A, P, B, B, B, A, P])["view_ring_passages"] == {pair(A, B), pair(A, P), pair(B, P)}
    assert W.coverage([A, P, B, B, B, A, P])["view_ring_shared"]
    assert W.coverage([P] * 6)["view_ring_passages"] == set() and W.coverage([P, A, B, P])["view_ring_passages"] == set()
    assert W.coverage([P, A, B, B, P, A, B, B, P])["view_ring_passages"] == set()  # every slot stays with its kind
    # the scene ring: every animated and accumulated launch uses it, whatever its size; animation against accumulate
    a3, blur, jit = ("animation3", -1), ("accumulate", 2), ("jitter", 5)
    assert W.coverage([a3, blur, jit, P, blur])["scene_ring_shared"]            # the fifth user takes the first one's slot
    assert W.coverage([blur, ("band", 0), a3, a3, ("batch66", 0), jit, A])["scene_ring_shared"]  # (plain launches use no scene table)
    assert not W.coverage([a3, blur, jit, P])["scene_ring_shared"]              # the ring never comes round
    assert not W.coverage([blur, jit, P, blur, jit, P, blur, blur])["scene_ring_shared"]  # one entry point, three kinds
    assert not W.coverage([a3, A, a3, A, A, a3])["scene_ring_shared"]
    assert not W.coverage([a3, blur, jit, A, a3, P, blur, A, A])["scene_ring_shared"]  # both in every window, every slot stays with its own
    # every PASS of a progressive kind is a user of the scene ring (two per launch), an entry point of its own
    prog, pj = ("progressive", 2), ("progressive_jitter", -1)
    pair = lambda a, b: frozenset((a, b))
    cov = W.coverage([("stream", 1), prog, ("stream", 0), pj, a3])   # users G G G G A: slot 0 passes from a pass to an animated launch
    assert cov["scene_ring_passages"] == {pair("progressive", "animation")} and not cov["scene_ring_shared"]
    assert cov["on_caller_stream"]["progressive"] == 1 and cov["on_caller_stream"]["progressive_jitter"] == 0
    cov = W.coverage([a3, a3, a3, prog, blur])                       # A A A G G U: A -> G (the second pass), A -> U
    assert cov["scene_ring_passages"] == {pair("animation", "progressive"), pair("animation", "accumulate")} and cov["scene_ring_shared"]
    cov = W.coverage([blur, a3, a3, a3, prog])                       # U A A A G G: U -> G, A -> G
    assert cov["scene_ring_passages"] == {pair("accumulate", "progressive"), pair("animation", "progressive")}
    assert W.coverage([blur, jit, blur, P, prog])["scene_ring_passages"] == {pair("accumulate", "progressive")}  # U U U U G G
    cov = W.coverage([a3, blur, a3, blur, a3, prog])                 # A U A U A G G: U -> G, A -> G, and never A against U
    assert cov["scene_ring_passages"] == {pair("accumulate", "progressive"), pair("animation", "progressive")}
    assert cov["scene_ring_shared"] is False
    assert W.coverage([a3, a3, a3, blur, blur])["scene_ring_shared"] and W.coverage([prog, pj, prog])["scene_ring_passages"] == set()
    assert W.scene_ring_users(W.trace([a3, ("band", 0), pj, P, prog])) == ["animation", "progressive", "progressive", "accumulate",
                                                                          "progressive", "progressive"]
    keys = W.linear_view_keys([("screen", 2), ("camera", 1), prog, pj])   # the views of the one-call twins
    assert keys == W.linear_view_keys([("screen", 2), ("camera", 1), blur, jit]) and len(keys) == 4 + 4
    # every PASS of a converging kind is a user too, under an entry point of its own: two of "converge" (C C), three of
    # "settle" (C C C); a trace is none
    conv, settle, tr = ("converge", 7), ("settle", 0), ("trace", 4)
    assert W.scene_ring_users(W.trace([a3, tr, conv, ("band", 0), settle, tr, prog, blur])) == \
        ["animation", "converge", "converge", "converge", "converge", "converge", "progressive", "progressive", "accumulate"]
    cov = W.coverage([("stream", 2), conv, tr, ("stream", 0), conv, a3, settle])   # users C C C C A C C C: C -> A, A -> C (one pair)
    assert cov["scene_ring_passages"] == {pair("converge", "animation")}
    assert cov["on_caller_stream"]["converge"] == 1 and cov["on_caller_stream"]["trace"] == 1 and cov["on_caller_stream"]["settle"] == 0
    cov = W.coverage([blur, a3, prog, tr, tr, settle])            # U A G G C C C: U -> C, A -> C, G -> C
    assert cov["scene_ring_passages"] == {pair("accumulate", "converge"), pair("animation", "converge"), pair("progressive", "converge")}
    assert W.coverage([settle, tr, conv, tr, settle])["scene_ring_passages"] == set()   # one entry point: no passage
    assert W.coverage([a3, tr, tr, tr, tr, blur, jit, P, settle])["scene_ring_passages"] == \
        {pair("animation", "converge"), pair("accumulate", "converge")}                  # (traces do not move the ring)
    assert W.coverage([("stream", 1), settle])["on_caller_stream"]["settle"] == 1
    # "converge": the four cameras through both cells, eight views per state; "settle" and "trace" need no linear view
    keys = W.linear_view_keys([("screen", 2), ("camera", 1), conv, ("converge", -1), settle, tr])
    assert len(keys) == 8 and {(k[1], k[6]) for k in keys} == {(cam, cell) for cam in range(W.N_CAMERAS) for cell in W.JITTER_CELLS}
    assert all(k[5] == W.morph_of(k[1]) for k in keys) and not W.linear_view_keys([("converge", 7)])  # (1024 x 512: beyond the model)
    views = W.converge_views(3)
    assert [v[0] for v in views] == [3, 0, 1, 2, 0, 1, 2, 3] and [v[2] for v in views] == list(W.JITTER_CELLS) * 4
    assert W.settle_views(2) == ([(2, 2), (3, 0), (0, 0)], [(3, 0), (0, 1), (1, 1)]) and W.trace_camera(3) == 0
    assert all(a != b for a, b in zip(*W.settle_views(1, 70)))  # every foreign view differs from its own


@pytest.mark.parametrize("ext", [0, 1])
@pytest.mark.parametrize("options", range(W.N_OPTIONS))
def test_pairs_are_the_plain_frames(options, ext, kifs, oracle):
    """What the "accumulate66" launches and Ctx.pairs of tests/test_gpu_context_lifecycle.py rest on, from the references
    alone: a frame of two equal sub-frames is (c + c) / 2 = c in f32, so accumulate_reference's frame is the oracle's
    plain frame byte for byte -- the three option sets, their own image and a morphed one, extensions off and on."""
    import accumulate_reference as ACC
    import test_gpu_context_lifecycle as L
    from helpers import oracle_uniforms
    K, O = kifs, oracle
    screen, cam, iters = K.ScreenData(64, 40), L._cameras(K)[1], L.ITERS[0]
    e = O.Ext(1, L.SHADOWS["shadow_steps"], L.SHADOWS["shadow_k"], L.SHADOWS["shadow_t0"], L.SHADOWS["shadow_max_t"]) if ext else None
    for m in (0, 1):
        image = L._morph(K, L._options(K)[options], m)
        frames = ACC.accumulate_frames(O, K, screen, [cam, cam], image, iters, 2, ext=e)
        s, c, o = oracle_uniforms(O, K, (screen, cam, L.Raw(image)))
        plain = O.render(s, c, o, O.iters(*iters), **(dict(ext=e) if ext else {}))
        assert frames.shape == (1, 40, 64, 4) and np.array_equal(frames[0], plain), (options, ext, m)
        # and Ctx.carried: the same two sub-frames as two passes through progressive_reference.fold, pass 1 at prior 0 over a
        # plane of NaNs, pass 2 at prior 1 -- the plain frame again, and the plane's w word is 2.0
        lin = ACC.linear_views(O, K, screen, [cam], image, iters, e)
        two, plane = L.carried_pair_model(O, lin)
        assert two.shape == (1, 40, 64, 4) and np.array_equal(two[0], plain), (options, ext, m)
        assert (plane[..., 3] == np.float32(2.0)).all() and not np.isnan(plane).any()
        assert (plane[..., :3].view(np.uint32) == (lin + lin).astype(np.float32).view(np.uint32)).all()
        _, mistaken = L.carried_pair_model(O, lin, prior_of_pass_2=0)  # (a pass 2 modelled at prior 0 would not pass the line above)
        assert (mistaken[..., 3] == np.float32(1.0)).all()


@pytest.mark.parametrize("ext", [0, 1])
@pytest.mark.parametrize("options", range(W.N_OPTIONS))
def test_settled_frames_are_the_plain_frames(options, ext, kifs, oracle):
    """What the "settle" launches and Ctx.settle of tests/test_gpu_context_lifecycle.py rest on, from the references
    alone (converge_reference.converged over the oracle's linear views): under the rule (0.0, 2) pass 1 leaves every
    pixel active (n = 1 < 2); pass 2 over the same views gives sums c + c, moment 2 Y(c)^2 and d = n q - L^2 = 0 <= 0
    exactly, so every pixel settles, the picture is the oracle's plain frame, the w word is 2.0 and the counts are 0;
    pass 3, handed a foreign view, marches nothing: the plain frame again, every bit of both planes kept.  The three
    option sets, their own image and a morphed one, extensions off and on."""
    import accumulate_reference as ACC
    import test_gpu_context_lifecycle as L
    from helpers import oracle_uniforms
    K, O = kifs, oracle
    screen, cams, iters = K.ScreenData(64, 40), L._cameras(K), L.ITERS[0]
    e = O.Ext(1, L.SHADOWS["shadow_steps"], L.SHADOWS["shadow_k"], L.SHADOWS["shadow_t0"], L.SHADOWS["shadow_max_t"]) if ext else None
    for m in (0, 1):
        image, other = L._morph(K, L._options(K)[options], m), L._morph(K, L._options(K)[options], (m + 1) % W.N_MORPHS)
        lin = ACC.linear_views(O, K, screen, [cams[1]], image, iters, e)
        foreign = ACC.linear_views(O, K, screen, [cams[2]], other, iters, e)
        assert (lin != foreign).any()
        s, c, o = oracle_uniforms(O, K, (screen, cams[1], L.Raw(image)))
        plain = O.render(s, c, o, O.iters(*iters), **(dict(ext=e) if ext else {}))
        one, two, three = L.settle_model(O, lin, foreign)
        assert one["counts"].tolist() == [64 * 40] and one["mask"].all()
        assert two["counts"].tolist() == [0] and two["mask"].all() and np.array_equal(two["frames"][0], plain), (options, ext, m)
        assert (two["sums"][..., 3] == np.float32(2.0)).all() and not np.isnan(two["sums"]).any() and not np.isnan(two["moments"]).any()
        assert (two["sums"][..., :3].view(np.uint32) == (lin + lin).astype(np.float32).view(np.uint32)).all()
        assert three["counts"].tolist() == [0] and not three["mask"].any() and np.array_equal(three["frames"][0], plain)
        assert (three["sums"].view(np.uint32) == two["sums"].view(np.uint32)).all()
        assert (three["moments"].view(np.uint32) == two["moments"].view(np.uint32)).all()
        # (a pass 3 modelled as marching would fold the foreign view in: other planes, another picture)
        mistaken = L.settle_model(O, lin, foreign, pass_3_marches=True)[2]
        assert mistaken["mask"].all() and (mistaken["sums"].view(np.uint32) != two["sums"].view(np.uint32)).any()
        assert not np.array_equal(mistaken["frames"][0], plain)


def test_the_converge_split_shows_in_the_model(kifs, oracle):
    """What Ctx.converge's comparisons rest on, from the references alone, at 64 x 40: under the rule of the walks the
    passes of 2 + 2 mask pixels (checked where Refs.converged builds a model), and a model with the pass sizes swapped
    -- 1 + 3 here, since 2 + 2 is its own mirror -- gives another pass 1 picture and other counts: the split is held."""
    import test_gpu_context_lifecycle as L
    K, O = kifs, oracle
    refs = L.Refs(K, O)
    want = refs.converged_on_host((64, 40), 1)
    assert len(want) == 2 and want[0]["sums"].shape == (W.CONVERGE_FRAMES, 40, 64, 4)
    lin = refs.converge_linear((64, 40), 1)
    other = L.converge_model(O, lin, splits=(1, 3), rule=W.CONVERGE_RULE)
    assert (other[0]["frames"] != want[0]["frames"]).any() and other[0]["counts"].tolist() != want[0]["counts"].tolist()
    assert {k: v for k, v in W.CONVERGING.items()} == {"converge": L.CONVERGE_SPLITS, "settle": (1,) * 3}
    assert L.CONVERGE_RULE == W.CONVERGE_RULE and L.SETTLE_RULE == W.SETTLE_RULE
    # a band's model is the rows of the frame's, the counts its own
    band = refs.converged_on_host((64, 40), 1, y0=7, y1=29)
    assert (band[1]["sums"].view(np.uint32) == want[1]["sums"][:, 7:29].view(np.uint32)).all()
    assert band[1]["counts"].tolist() == [int(m.sum()) for m in CR_active_rows(want[1], 7, 29)]


def CR_active_rows(state, y0, y1):
    """Per frame the pixels of rows [y0, y1) still active in a pass's state, under the walks' rule and pass size."""
    import converge_reference as CR
    left = CR.active(state["sums"][:, y0:y1], state["moments"][:, y0:y1], W.CONVERGE_RULE, W.CONVERGING["converge"][1])
    return [left[f] for f in range(left.shape[0])]


def test_the_progressive_split_shows_in_the_model(kifs, oracle):
    """What Ctx.progressive's comparisons rest on, from the references alone, at 64 x 40: the final plane and picture of
    the blur views are the same bits for the splits 1 + 2 and 2 + 1 (the fold is one sum in one order), so it is pass 1's
    picture that holds the split -- for 1 + 2 the plain frame of every frame's first sub-frame, and another picture for
    2 + 1.  A model with the two pass sizes swapped fails the comparison of pass 1's picture."""
    import accumulate_reference as ACC
    import test_gpu_context_lifecycle as L
    from helpers import oracle_uniforms
    K, O = kifs, oracle
    screen, cams, gui, iters = K.ScreenData(64, 40), L._cameras(K), L._options(K)[0], L.ITERS[0]
    views, samples, splits = L.progressive_views("blur", 1)
    assert (samples, splits) == (3, (1, 2)) and len(views) == 6
    lin = np.stack([ACC.linear_views(O, K, screen, [cams[cam]], L._morph(K, gui, m), iters, None)[0] for cam, m, _ in views])
    frames, plane = L.progressive_model(O, lin, samples, splits)
    swapped, swapped_plane = L.progressive_model(O, lin, samples, splits[::-1])
    assert (plane.view(np.uint32) == swapped_plane.view(np.uint32)).all() and np.array_equal(frames[-1], swapped[-1])
    assert (frames[0] != swapped[0]).any(-1).sum() * 100 >= 64 * 40
    for f in range(2):
        cam, m, _ = views[f * samples]
        s, c, o = oracle_uniforms(O, K, (screen, cams[cam], L.Raw(L._morph(K, gui, m))))
        assert np.array_equal(frames[0][f], O.render(s, c, o, O.iters(*iters)))
    assert L.progressive_views("jitter", 1)[1:] == (2, (1, 1))
    # the walks' kinds and Ctx.progressive's agree on the passes
    assert {k: (sum(v), v) for k, v in W.PROGRESSIVE.items()} == {k: L.PROGRESSIVE_SPLITS[L.PROGRESSIVE_KINDS[k]] for k in W.PROGRESSIVE}
