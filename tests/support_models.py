"""NumPy models of the kernels around the render kernels (csrc/kifs_support_kernels.hip), written from the contract in
include/kifs_hip.h ("row shards", "sparse shards") and from nothing else: no product code is imported here.

Every buffer is a flat uint8 array -- a whole allocation -- and a Layout says where the library's view of it lies:
frame (or shard) i starts at byte base + i * stride and its row r at + r * pitch.  The models change exactly the bytes the
contract names and no others, so comparing whole allocations also checks guards, pitch padding and the gaps between frames.
Pixels are little-endian RGBA8 words.  Plain loops over stripes, rows and tiles: clarity over speed, the shapes are small."""
from collections import namedtuple

import numpy as np

Layout = namedtuple("Layout", "base pitch stride")

STRIPE_ROWS = 8         # KIFS_STRIPE_ROWS
TILE_W = 32
RECORD_WORDS = 260      # KIFS_SPARSE_RECORD_BYTES / 4: tile id, three zero words, 8 x 32 pixels
BINS = 1024


def stripe_rows(stripe, H):
    """Rows of stripe `stripe` that lie in a frame of H rows."""
    return min(STRIPE_ROWS, H - stripe * STRIPE_ROWS)


def tiles_x(W):
    return (W + TILE_W - 1) // TILE_W


def get_words(buf, at, n):
    """n pixels at byte `at` of buf, as uint32 (a copy: `at` need not be aligned in the host array)."""
    return buf[at:at + 4 * n].copy().view("<u4")


def put_words(buf, at, words):
    buf[at:at + 4 * len(words)] = np.ascontiguousarray(words, dtype="<u4").view(np.uint8)


def unpack_stripes(frames, shards, layouts, stripes, W, H, count):
    """kifs_unpack_shard_async: stripe k of packed shard i (its rows [8 k, 8 k + 8)) -> frame i's rows [8 stripes[k], ..),
    clipped to H; 4 W bytes per row.  layouts = (frame layout, shard layout).  Changes `frames` in place."""
    fl, sl = layouts
    for i in range(count):
        for k, s in enumerate(stripes):
            for r in range(stripe_rows(s, H)):
                src = sl.base + i * sl.stride + (STRIPE_ROWS * k + r) * sl.pitch
                dst = fl.base + i * fl.stride + (STRIPE_ROWS * s + r) * fl.pitch
                frames[dst:dst + 4 * W] = shards[src:src + 4 * W]
    return frames


def fill_stripes(frames, layout, stripes, W, H, count, bg):
    """kifs_fill_shard_async: the pixel `bg` over the rows of the listed stripes of `count` frames."""
    row = np.full(W, bg, dtype="<u4")
    for i in range(count):
        for s in stripes:
            for r in range(stripe_rows(s, H)):
                put_words(frames, layout.base + i * layout.stride + (STRIPE_ROWS * s + r) * layout.pitch, row)
    return frames


def pack_sparse(shards, layout, stripes, W, H, count, bg):
    """kifs_pack_sparse_async: (n, 260) uint32 records, sorted by tile id.  A record is [id, 0, 0, 0, 256 pixels row by
    row]; id = (shard * n_stripes + stripe slot) * tiles_x + tile column.  Pixels outside the frame, or below the last row
    of a partial stripe, hold bg; a tile gets a record iff one of its IN-FRAME pixels differs from bg."""
    tx, records = tiles_x(W), []
    for i in range(count):
        for k, s in enumerate(stripes):
            rows = stripe_rows(s, H)
            for c in range(tx):
                w = min(TILE_W, W - c * TILE_W)
                tile = np.full((STRIPE_ROWS, TILE_W), bg, dtype="<u4")
                for r in range(rows):
                    tile[r, :w] = get_words(shards, layout.base + i * layout.stride + (STRIPE_ROWS * k + r) * layout.pitch
                                            + 4 * c * TILE_W, w)
                if (tile != np.uint32(bg)).any():  # (everything outside the frame is bg by construction)
                    rec = np.zeros(RECORD_WORDS, dtype="<u4")
                    rec[0] = (i * len(stripes) + k) * tx + c
                    rec[4:] = tile.ravel()
                    records.append(rec)
    return np.array(records, dtype="<u4").reshape(-1, RECORD_WORDS)


def unpack_sparse(frames, layout, records, stripes, W, H, count, erase=False, bg=None):
    """kifs_unpack_sparse_async (erase: kifs_erase_sparse_async, which writes bg instead of the record's pixels): every
    record, in order, to its tile of its frame, clipped to W and H; records whose id is not below
    count * n_stripes * tiles_x are skipped."""
    tx = tiles_x(W)
    for rec in np.asarray(records, dtype="<u4").reshape(-1, RECORD_WORDS):
        tid = int(rec[0])
        if tid >= count * len(stripes) * tx:
            continue
        i, rest = divmod(tid, len(stripes) * tx)
        k, c = divmod(rest, tx)
        w = min(TILE_W, W - c * TILE_W)
        tile = np.full((STRIPE_ROWS, TILE_W), bg, dtype="<u4") if erase else rec[4:].reshape(STRIPE_ROWS, TILE_W)
        for r in range(stripe_rows(stripes[k], H)):
            put_words(frames, layout.base + i * layout.stride + (STRIPE_ROWS * stripes[k] + r) * layout.pitch + 4 * c * TILE_W,
                      tile[r, :w])
    return frames


def tile_bins(cost, shift):
    """Bin of every tile in the tile-order sort: 1023 - min(cost >> shift, 1023); bin 0 (the heaviest) goes first."""
    c = np.asarray(cost, dtype=np.uint32).astype(np.uint64) >> np.uint64(shift)
    return (BINS - 1 - np.minimum(c, BINS - 1)).astype(np.int64)


def tile_ids(n, tiles_x_):
    """What a tile order is a permutation of: tile i as (column | row << 16)."""
    i = np.arange(n, dtype=np.uint64)
    return ((i % np.uint64(tiles_x_)) | ((i // np.uint64(tiles_x_)) << np.uint64(16))).astype(np.uint32)
