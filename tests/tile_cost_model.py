"""NumPy models of what the tile order's feedback records and sorts (kifs_render_common.hpp: cost_from_work;
kifs_support_kernels.hip: tile_order_kernel with its memory; kifs_schedule.cpp: work_cost_shift), shared by
test_tile_cost_model.py (CPU) and test_gpu_tile_cost.py."""
import numpy as np

BINS = 1024
WORK_PER_SHADED_CHUNK = 8
COST_TOP = 1 << 20
SEEN_COST_MAX = (1 << 24) - 1
ORDER_WINDOW_BATCH = 16  # rules::ORDER_WINDOW_BATCH


def cost_from_work(march_steps, hits):
    """A tile's recorded cost in the throughput kernels: the march steps of every chunk-round of its wave or workgroup,
    plus a fixed term per chunk of 64 hits shaded; saturating."""
    return min(int(march_steps) + WORK_PER_SHADED_CHUNK * ((int(hits) + 63) >> 6), COST_TOP)


def wave_tile_work(steps_per_ray, round_steps, max_iterations):
    """The march steps render_wave_kernel's wave runs for one tile whose live rays stop after steps_per_ray[i] >= 1 steps
    (the step at which a ray hits, leaves or runs out counts): rounds of `round_steps` steps over chunks of 64 rays, the
    survivors re-queued; the last chunk is marched to its end in one go; a chunk-round lasts until its last ray stops."""
    left = np.sort(np.asarray(steps_per_ray, dtype=np.int64))
    trips, work = 0, 0
    while left.size:
        limit = max_iterations if left.size <= 64 else min(trips + round_steps, max_iterations)
        for c0 in range(0, left.size, 64):  # (which rays share a chunk does not change the sum's bound, only the sum: the
            chunk = left[c0:c0 + 64]        #  model takes the queue sorted, the kernel's is in arrival order)
            work += int(min(chunk.max(), limit) - trips)
        left = left[left > limit]
        trips = limit
    return work


def group_work(steps_per_ray, round_steps, max_iterations, marches_last_chunk_to_the_end=True):
    """The march steps render_group_kernel counts for the rays of its tiles: a round of several chunks counts every chunk for
    the round's whole length (its chunks are drawn by ticket, so which rays share one is not fixed), a single chunk the
    steps it ran.  The generalised Julia pipeline keeps rounds to the end (marches_last_chunk_to_the_end False)."""
    left = np.asarray(steps_per_ray, dtype=np.int64)
    trips, work = 0, 0
    while left.size:
        one = left.size <= 64
        limit = max_iterations if (one and marches_last_chunk_to_the_end) else min(trips + round_steps, max_iterations)
        work += int(min(left.max(), limit) - trips) if one else -(-left.size // 64) * (limit - trips)
        left = left[left > limit]
        trips = limit
    return work


def work_cost_shift(max_iterations, group_tiles, round_steps=16):
    """The sort's shift for recorded work: the top of the range -- 4 chunks per tile x (max_iterations + one shaded chunk)
    -- must land in the 1024 bins.  0 for a launch without rounds (run times, sorted as they are)."""
    if round_steps <= 0:
        return 0
    top = 4 * max(group_tiles, 1) * (max(max_iterations, 0) + WORK_PER_SHADED_CHUNK)
    shift = 0
    while shift < 31 and (top >> shift) > BINS - 1:
        shift += 1
    return shift


def remember(seen, cost, window):
    """One sort's update of the memory: seen = cost << 8 | age keeps every tile's largest cost of the last `window` sorts;
    a cost at least as large, or an entry `window` sorts old, replaces it."""
    seen = np.asarray(seen, dtype=np.uint32)
    now = np.minimum(np.asarray(cost, dtype=np.uint32), np.uint32(SEEN_COST_MAX))
    age = (seen & np.uint32(0xff)) + np.uint32(1)
    fresh = (now >= (seen >> np.uint32(8))) | (age >= np.uint32(window))
    return np.where(fresh, now << np.uint32(8), (seen & ~np.uint32(0xff)) | age).astype(np.uint32)


def bins_of(keys, shift):
    return (BINS - 1) - np.minimum(np.asarray(keys, dtype=np.uint32) >> np.uint32(shift), np.uint32(BINS - 1)).astype(np.int64)


def stable_order(keys, shift, tiles_x):
    """Tile ids (x | y << 16), heaviest bin first, ties in index order: the order tile_order_kernel's stable scatter gives."""
    idx = np.argsort(bins_of(keys, shift), kind="stable")
    return ((idx % tiles_x) | ((idx // tiles_x) << 16)).astype(np.uint32)


def bins_along(order, keys, shift, tiles_x):
    """The bins of the tiles in the sequence `order` lists them."""
    index = (order & 0xffff).astype(np.int64) + (order >> 16).astype(np.int64) * tiles_x
    return bins_of(keys, shift)[index]


def wave_queue_work(steps_in_arrival_order, round_steps, max_iterations):
    """render_wave_kernel's march steps for one tile, EXACTLY: `steps_in_arrival_order` lists the live rays' step counts in
    the order round 0 queues them (8 x 8 block by block, lane by lane); every round takes its chunks of 64 from the top of
    the queue down, a chunk-round lasts until its last ray stops or the round ends, survivors are filed in the order they
    were marched; a queue of one chunk is marched to the end."""
    queue = [int(s) for s in steps_in_arrival_order]
    trips, work = 0, 0
    while queue:
        n = len(queue)
        limit = max_iterations if n <= 64 else min(trips + round_steps, max_iterations)
        nxt = []
        for c0 in range(((n - 1) >> 6) << 6, -1, -64):
            chunk = queue[c0:c0 + 64]
            work += min(max(chunk), limit) - trips
            nxt.extend(s for s in chunk if s > limit)
        queue, trips = nxt, limit
    return work


def wave_arrival_order(valid):
    """Indices (ly, lx) of a 8 x 32 tile's pixels in the order render_wave_kernel queues them: block b = lx // 8 by block,
    lane = ly * 8 + lx % 8; `valid[ly][lx]`: inside the frame."""
    return [(lane >> 3, (b << 3) | (lane & 7)) for b in range(4) for lane in range(64) if valid[lane >> 3][(b << 3) | (lane & 7)]]
