"""Seeded walks over the state of one long-lived context (tests/test_gpu_context_lifecycle.py::test_seeded_walk).

plan(seed) is a pure function of the seed: a list of 104 operations, each a tuple (kind, argument).  The GPU test replays
it on one GraphicState and checks every render; tests/test_context_walk_plan.py (CPU) replays it on the model below --
the context's eight tile-table slots, least recently used replaced (kifs_schedule.cpp, tile_table) -- and asserts what a
walk must cover.  Nothing here touches the library.

Besides the plain launches (bands, batches, shards, geometry) a walk holds the two entry points with state of their own
between launches: "adaptive" (kifs_render_adaptive_async: the scratch block and its event / stream pair) and
"animation3" / "animation66" (kifs_render_animation_async: the scene-table ring, the view-table ring it shares with
"batch66", its own stream rule on the tile table).  Frame j of an animated launch uses camera batch_cameras(camera, n)[j]
and the option image morph_of(that camera) of the context's options, so that a launch's frames differ in scene as well
as in view and still need no more than four references per context state.

The accumulated launches (kifs_render_accumulate_async and kifs_render_accumulate_jittered_async) share both rings with
them and write the tile table's last_stream as they do: "accumulate" is a blur launch of 2 frames x 3 sub-frames on the
whole frame or a band, "jitter" one of 2 x 2 on a grid of 2, and "accumulate66" 33 frames of 2 identical sub-frames each
-- 66 views, a third user of the view-table ring, whose frames are the oracle's plain frames.  The cameras are
batch_cameras(camera, views) and every sub-frame carries the option image morph_of(its camera), so a context state needs
at most four linear views for blur and eight for jitter (linear_view_keys counts them per plan).

Progressive accumulation (kifs_render_accumulate_resume_async) goes through the same rings, tile tables, last_stream and
options scope, and a progressive frame is the one result that depends on several launches: "progressive" renders the
views of an "accumulate" launch as two passes of 1 + 2 sub-frames per frame over a plane of the test's own, and
"progressive_jitter" those of a "jitter" launch as 1 + 1, with a lone launch of the same rows and the context's camera
between the passes.  Every PASS is a user of the scene ring (scene_ring_users); a kind takes the table key of the band or
frame it renders and the linear views of its one-call twin (AS_ONE_CALL), so its model costs nothing the twin's did not.

Converging accumulation (kifs_render_accumulate_converge_async) goes the same way and adds a per-pixel mask derived from
two planes.  "converge": 2 frames x 4 sub-frames on the grid JITTER_GRID as two passes of 2 + 2 under the rule
CONVERGE_RULE, on the whole frame or a band; sub-frame s of frame f has camera (camera + f + s) % N_CAMERAS, the option
image of that camera and cell JITTER_CELLS[s % 2] (converge_views) -- the four cameras through both cells, eight linear
views per context state.  "settle" is exact at any size: the whole frame, 3 frames x 1 sub-frame, three passes under
SETTLE_RULE = (0.0, 2).  Pass 1 restarts without a picture (n = 1 < 2: everything stays active); pass 2 takes the same
views, so that the sums are c + c, the moment 2 Y(c)^2 and d = n q - L^2 = 0 <= 0 exactly: every pixel settles, the
picture is the oracle's plain frame, the counts fall from W * H to 0; pass 3 is handed FOREIGN views (settle_views) and
must march nothing.  Every pass of both is a user of the scene ring under the entry point "converge".  "trace" is a ray
query (kifs_trace_rays_async): the pixel rays of the rows of a band for camera (camera + 1) % N_CAMERAS -- not the
context's, which the call must not read -- under the context's options, iteration counts and extensions, also while
supersampling is 2.  It takes no tile table and no ring.  Between the passes of "converge" and "settle" lies a lone
launch of the same rows and a trace of them.
"""
import random

SIZES = ((1024, 512), (330, 149), (64, 40), (1056, 516), (200, 135))  # 2048 tiles (feedback), ragged, tiny, 33 x 65, small
N_CAMERAS, N_OPTIONS, N_ITERS, N_BANDS, N_STREAMS = 4, 3, 2, 12, 3
N_MORPHS = 3  # option images per option set: 0 the set itself, 1 and 2 with other constant, power and colours
TABLE_SLOTS = 8  # MAX_TILE_TABLES of kifs_context.hpp
VIEW_RING = 4    # kifs_ctx::VIEW_RING: the view tables of launches beyond 64 views
SCENE_RING = 4   # kifs_ctx::SCENE_RING: the scene tables of animated and accumulated launches
MODEL_UP_TO = (330, 149)  # the largest screen a launch is held to a per-pixel model of the oracle on
STEPS = 104
# Searched 0..19999 at 104 steps: 15 seeds meet tests/test_context_walk_plan.py (3757, 3876, 3974, 5025, 5108, 5208, 5673, 9353,
# 9535, 11094, 11877, 14567, 15086, 17037, 19124; at 88 steps, the count before the converging kinds and the ray query joined,
# none of the 20000 does, at 96 three, at 112 forty-nine).  These three need 4, 4 and 20 linear views and between them run
# "converge" against its model at 64 x 40 and 330 x 149, whole frames and a band, and against a fresh context at 1024 x 512
# and 1056 x 516, "settle" at three sizes, and all three kinds on the context's and on caller streams.  (14567 needs no
# linear view because no modelled size sees an accumulated launch; 3876 never leaves 1024 x 512; 17037, with 16 views of
# which 8 are 330 x 149, made a walk of 4 s, most of it the references.)
SEEDS = (3757, 9353, 19124)

# kind -> (weight, arguments to draw from); the renders outweigh the state changes so that the set of distinct
# (scene, camera, size) references stays small
OPS = {
    "screen": (3, range(len(SIZES))),
    "camera": (3, range(N_CAMERAS)),
    "options": (2, range(N_OPTIONS)),
    "iters": (2, range(N_ITERS)),
    "extensions": (2, (0, 1)),
    "supersampling": (2, (1, 2)),
    "frames_in_flight": (2, (1, 3)),
    "band": (14, range(N_BANDS)),
    "batch3": (3, (0,)),
    "batch66": (2, (0,)),
    "shard": (3, (0, 1, 2)),      # the rank of three whose stripes are rendered
    "geometry": (3, (0,)),
    "stream": (2, range(N_STREAMS)),  # 0: the context's stream, 1 / 2: caller streams
    "adaptive": (3, (2, 3)),          # k; the thresholds are adaptive_reference.DEFAULT
    "animation3": (3, (-1, 2, 7)),    # -1: the whole frame, else the band band_rows(h, argument)
    "animation66": (2, (0,)),         # the whole frame, 66 frames: beyond MAX_BATCH_INLINE
    "accumulate": (3, (-1, 2, 7)),    # blur, 2 frames x 3 sub-frames; the rows as "animation3"
    "jitter": (3, (-1, 5)),           # 2 frames x 2 sub-frames through cells JITTER_CELLS of a grid of 2; the rows likewise
    "accumulate66": (2, (0,)),        # pairs: 33 frames x 2 equal sub-frames = 66 views, the whole frame
    "progressive": (3, (-1, 2, 7)),   # the views of "accumulate" as passes of 1 + 2 sub-frames per frame; the rows likewise
    "progressive_jitter": (2, (-1, 5)),  # the views of "jitter" as passes of 1 + 1, a picture from both; the rows likewise
    "converge": (3, (-1, 2, 7)),      # 2 frames x 4 sub-frames as converging passes of 2 + 2; the rows as "animation3"
    "settle": (2, (0,)),              # the whole frame, 3 frames x 1 sub-frame, three converging passes: exact at any size
    "trace": (4, range(N_BANDS)),     # a ray query: the pixel rays of the band's rows, camera (camera + 1) % N_CAMERAS
}
ACCUMULATED = {"accumulate": (2, 3), "jitter": (2, 2), "accumulate66": (33, 2)}  # kind -> (frames, sub-frames per frame)
RENDERS = ("band", "batch3", "batch66", "shard", "geometry", "adaptive", "animation3", "animation66") + tuple(ACCUMULATED)
# refused by the API while supersampling > 1
ONE_SAMPLE_ONLY = ("geometry", "adaptive", "animation3", "animation66") + tuple(ACCUMULATED)
STATEFUL = ("adaptive", "animation3", "animation66") + tuple(ACCUMULATED)  # entry points with state of their own
ANIMATED = {"animation3": 3, "animation66": 66}                          # kind -> frames
VIEW_RING_USERS = ("batch66", "animation66", "accumulate66")
PROGRESSIVE = {"progressive": (1, 2), "progressive_jitter": (1, 1)}  # kind -> sub-frames per frame of every pass
AS_ONE_CALL = {"progressive": "accumulate", "progressive_jitter": "jitter"}  # the launch whose views, rows and model a kind shares
RENDERS += tuple(PROGRESSIVE)
ONE_SAMPLE_ONLY += tuple(PROGRESSIVE)
STATEFUL += tuple(PROGRESSIVE)
JITTER_GRID, JITTER_CELLS = 2, ((1, 0), (0, 1))  # sub-frame s of every frame of a "jitter" launch goes through JITTER_CELLS[s]
CONVERGING = {"converge": (2, 2), "settle": (1, 1, 1)}  # kind -> sub-frames per frame of every converging pass
CONVERGE_FRAMES, SETTLE_FRAMES = 2, 3
# (tolerance, min_samples) of every pass of the kind.  The tolerance is 3/32 and not 1/16: two option images of one set
# differ in their background's luminance by between 1/8 and 3/16, which is 2 x tolerance for two samples, so at 1/16 a
# frame whose first pass pairs two such images keeps its whole background active and no 8 x 8 block of it is empty
# (asserted from the model alone where Refs.converged of tests/test_gpu_context_lifecycle.py builds one).  From the model
# alone: 3/32 meets those assertions for every modelled "converge" of 14 of the 15 qualifying seeds and for option set 0
# at the three modelled sizes and all four cameras; 1/16 fails half of the latter, 1/8 one more seed, 5/32 and 3/16 more.
CONVERGE_RULE, SETTLE_RULE = (3.0 / 32.0, 2), (0.0, 2)
RENDERS += tuple(CONVERGING) + ("trace",)
ONE_SAMPLE_ONLY += tuple(CONVERGING)  # (a trace is the one call the API takes while supersampling > 1)
STATEFUL += tuple(CONVERGING) + ("trace",)  # (a trace keeps nothing; it borrows the context's screen, camera and factor)


def morph_of(camera_index):
    """The option image an animated launch gives the frame of this camera."""
    return camera_index % N_MORPHS


def band_rows(height, i):
    """Band i of 12: a quarter of the frame starting at sixteenths, neither end on a tile row for most heights."""
    return (i * height) // 16, ((i + 4) * height) // 16 + (1 if i % 2 else 0)


def animation_rows(height, arg):
    """The rows of an "animation3", "accumulate" or "jitter" launch: the whole frame for -1, else band `arg`."""
    return (0, height) if arg < 0 else band_rows(height, arg)


def shard_stripes(height, rank):
    """Stripes rank, rank + 3, ... of the frame's 8-row stripes (equal shares of kifs_shard_stripes for a world of 3)."""
    return tuple(range(rank, (height + 7) // 8, 3))


def plan(seed):
    rng = random.Random(seed)
    kinds = list(OPS)
    weights = [OPS[k][0] for k in kinds]
    ops, supersampling = [], 1
    while len(ops) < STEPS:
        kind = rng.choices(kinds, weights)[0]
        arg = rng.choice(list(OPS[kind][1]))
        if kind in ONE_SAMPLE_ONLY and supersampling > 1:
            continue  # refused by the API: a resolved pixel has no single hit, and the newer calls take one sample
        if kind == "supersampling":
            supersampling = arg
        ops.append((kind, arg))
    return ops


def trace(ops):
    """(op index, kind, argument, state) for every render of a plan (a ray query among them); state is the context's configuration at that
    point: size, camera, options, iters, extensions, supersampling, frames_in_flight and stream, as indices."""
    state = dict(size=0, camera=0, options=0, iters=0, extensions=0, supersampling=1, frames_in_flight=1, stream=0)
    for i, (kind, arg) in enumerate(ops):
        if kind in RENDERS:
            yield i, kind, arg, dict(state)
        else:
            state["size" if kind == "screen" else kind] = arg


def batch_cameras(camera, n):
    """The views of a batch: the four cameras in turn, starting at the context's."""
    return [(camera + j) % N_CAMERAS for j in range(n)]


def replay(ops):
    """The tile-table geometries a plan visits: yields (op index, key, event) for every render, event one of "hit",
    "fill" (an empty slot), "evict" and "return" (a miss on a geometry this walk has evicted before: also an eviction).
    An animated or accumulated band takes the table of the plain band of its rows; an adaptive call's first pass and a
    whole-frame animated or accumulated launch take the full frame's.  A progressive kind takes the key of the band or
    frame it renders, as its one-call twin; the lone launch between its passes renders the same rows -- a hit.  So do
    "converge" (a band or the frame) and "settle" (the frame); a "trace" takes no tile table and is skipped."""
    size = SIZES[0]
    slots, clock, evicted = {}, 0, set()
    for i, (kind, arg) in enumerate(ops):
        if kind == "screen":
            size = SIZES[arg]
        if kind not in RENDERS or kind == "trace":
            continue
        kind = AS_ONE_CALL.get(kind, kind)
        w, h = size
        if kind == "band" or (kind in ("animation3", "accumulate", "jitter", "converge") and arg >= 0):
            key = (w, h) + band_rows(h, arg) + (None,)
        elif kind == "shard":
            key = (w, h, 0, h, shard_stripes(h, arg))
        else:
            key = (w, h, 0, h, None)
        clock += 1
        if key in slots:
            event = "hit"
        elif len(slots) < TABLE_SLOTS:
            event = "fill"
        else:
            victim = min(slots, key=slots.get)
            del slots[victim]
            evicted.add(victim)
            event = "return" if key in evicted else "evict"
        slots[key] = clock
        yield i, key, event


def modelled(size):
    return size[0] <= MODEL_UP_TO[0] and size[1] <= MODEL_UP_TO[1]


def blur_views(camera):
    """(camera, option image) of the six sub-frames of an "accumulate" launch, frame by frame."""
    return [(cam, morph_of(cam)) for cam in batch_cameras(camera, 6)]


def jitter_views(camera):
    """(camera, option image, cell) of the four sub-frames of a "jitter" launch, frame by frame."""
    return [(cam, morph_of(cam), JITTER_CELLS[v % 2]) for v, cam in enumerate(batch_cameras(camera, 4))]


def converge_views(camera):
    """(camera, option image, cell) of the eight sub-frames of a "converge" frame pair, frame by frame: sub-frame s of
    frame f has camera (camera + f + s) % N_CAMERAS."""
    return [(cam, morph_of(cam), JITTER_CELLS[s % 2]) for f in range(CONVERGE_FRAMES)
            for s, cam in enumerate(batch_cameras(camera + f, sum(CONVERGING["converge"])))]


def settle_views(camera, n=SETTLE_FRAMES):
    """((camera, option image) of the n frames of a "settle" in passes 1 and 2, the FOREIGN ones handed to pass 3: every
    frame's camera + 1 and the next option image)."""
    own = [(cam, morph_of(cam)) for cam in batch_cameras(camera, n)]
    return own, [((cam + 1) % N_CAMERAS, (m + 1) % N_MORPHS) for cam, m in own]


def trace_camera(camera):
    """The camera whose pixel rays a "trace" is handed: never the context's own."""
    return (camera + 1) % N_CAMERAS


def linear_view_keys(ops):
    """The distinct per-pixel linear views (size, camera, options, iters, extensions, option image, cell) the blur,
    jitter and "converge" launches of a plan are modelled from: the cost of their references, known before a GPU run.  cell is None for
    blur; screens beyond MODEL_UP_TO need none (there the launch is compared with a fresh context's)."""
    keys = set()
    for _, kind, _, st in trace(ops):
        size = SIZES[st["size"]]
        kind = AS_ONE_CALL.get(kind, kind)  # the passes of a progressive frame render its twin's views
        if kind in ("accumulate", "jitter", "converge") and modelled(size):
            views = {"accumulate": lambda c: [v + (None,) for v in blur_views(c)], "jitter": jitter_views,
                     "converge": converge_views}[kind](st["camera"])
            keys |= {(size, cam, st["options"], st["iters"], st["extensions"], m, cell) for cam, m, cell in views}
    return keys


def _passages(users, ring):
    """The unordered pairs of different users of which one takes a ring's slot from the other: user n and user n + ring."""
    return {frozenset((users[i], users[i + ring])) for i in range(len(users) - ring) if users[i] != users[i + ring]}


def scene_ring_users(renders):
    """The users of the scene ring in a plan's renders, in order, by entry point: every animated launch ("animation"),
    every accumulated launch ("accumulate"), every PASS of a progressive kind ("progressive") and every PASS of a
    converging kind ("converge": two of "converge", three of "settle").  A "trace" uses no ring."""
    users = []
    for _, kind, _, _ in renders:
        if kind in ANIMATED or kind in ACCUMULATED:
            users.append("animation" if kind in ANIMATED else "accumulate")
        elif kind in PROGRESSIVE:
            users += ["progressive"] * len(PROGRESSIVE[kind])
        elif kind in CONVERGING:
            users += ["converge"] * len(CONVERGING[kind])
    return users


def coverage(ops):
    """What a plan exercises: launches per kind, evictions and returns of the table model, per entry point with state of
    its own the launches made while the walk's stream is a caller's (1 or 2), and how the two rings are shared.  A user
    of a ring and the user four later take the same slot.  view_ring_passages: the pairs of kinds of VIEW_RING_USERS
    between which a view-table slot passes, in either order; view_ring_shared: "batch66" and "animation66" are one of
    them.  scene_ring_shared: among the users of the scene ring -- every animated and every accumulated launch -- some
    user and the user SCENE_RING later belong to different entry points, animation against accumulate.
    scene_ring_passages: the pairs of entry points of scene_ring_users -- every pass of a progressive kind a user of its
    own -- between which a scene-table slot passes."""
    events = [e for _, _, e in replay(ops)]
    kinds = {k: sum(1 for kind, _ in ops if kind == k) for k in OPS}
    renders = list(trace(ops))
    on_caller_stream = {k: sum(1 for _, kind, _, st in renders if kind == k and st["stream"] in (1, 2)) for k in STATEFUL}
    passages = _passages([kind for _, kind, _, _ in renders if kind in VIEW_RING_USERS], VIEW_RING)
    scene_passages = _passages(scene_ring_users(renders), SCENE_RING)
    return {"kinds": kinds, "evictions": events.count("evict") + events.count("return"), "returns": events.count("return"),
            "on_caller_stream": on_caller_stream, "view_ring_passages": passages,
            "view_ring_shared": frozenset(("batch66", "animation66")) in passages,
            "scene_ring_shared": frozenset(("animation", "accumulate")) in scene_passages, "scene_ring_passages": scene_passages}
