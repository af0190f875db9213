"""The five kernels around the render kernels (csrc/kifs_support_kernels.hip) -- unpack_stripes, pack_sparse,
unpack_sparse with its erase mode, fill_stripes, tile_order -- against the NumPy models of tests/support_models.py,
through the C ABI itself: the Python wrappers only ever pass tight pitches and contiguous, 16-byte aligned tensors,
which selects the 16-byte code path of every kernel and never the 4-byte one.

Every buffer is a flat uint8 device allocation, pre-filled with a canary byte, with GUARD bytes in front of and behind
the view the library is given; the view starts at a chosen offset and has a chosen pitch and stride.  After every call
the WHOLE allocation must equal the model's whole allocation: guards, pitch padding, the gaps between frames, the rows
of stripes that were not listed and the record space beyond n_records are all compared.  Nothing here has a tolerance.

CASES is a literal table; test_case_table_covers_the_code_paths (no GPU needed) checks what it must contain."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import support_models as M
from helpers import oracle_frame

gpu = pytest.mark.gpu

CANARY = 0xA5
GUARD = 256  # bytes in front of and behind every view; a multiple of 16
BAD_SIZE, BAD_ARG = 3, 7
LAYOUTS = ("tight16", "offset4", "pitch+4", "padded16", "stride+4")
STRIPE_LISTS = ("all", "rank1of3", "weighted", "last", "first")

# (W, H, frame layout, shard layout, stripe list, count).  The widths 2 and 34 are here for W % 4 == 2.
CASES = [
    (1, 1, 'tight16', 'tight16', 'all', 1),
    (1, 1, 'offset4', 'offset4', 'rank1of3', 3),
    (1, 1, 'pitch+4', 'pitch+4', 'weighted', 1),
    (1, 1, 'stride+4', 'stride+4', 'last', 3),
    (3, 7, 'tight16', 'offset4', 'rank1of3', 3),
    (3, 7, 'offset4', 'pitch+4', 'weighted', 1),
    (3, 7, 'pitch+4', 'stride+4', 'last', 3),
    (3, 7, 'stride+4', 'tight16', 'first', 3),
    (4, 8, 'tight16', 'padded16', 'weighted', 1),
    (4, 8, 'offset4', 'padded16', 'last', 3),
    (4, 8, 'pitch+4', 'stride+4', 'first', 3),
    (4, 8, 'padded16', 'tight16', 'all', 3),
    (4, 8, 'stride+4', 'offset4', 'rank1of3', 3),
    (5, 9, 'tight16', 'stride+4', 'last', 3),
    (5, 9, 'offset4', 'tight16', 'first', 1),
    (5, 9, 'pitch+4', 'offset4', 'all', 3),
    (5, 9, 'stride+4', 'pitch+4', 'rank1of3', 3),
    (31, 7, 'tight16', 'tight16', 'first', 1),
    (31, 7, 'offset4', 'offset4', 'all', 3),
    (31, 7, 'pitch+4', 'pitch+4', 'rank1of3', 1),
    (31, 7, 'stride+4', 'stride+4', 'weighted', 3),
    (32, 8, 'tight16', 'tight16', 'all', 3),
    (32, 8, 'offset4', 'offset4', 'rank1of3', 1),
    (32, 8, 'pitch+4', 'pitch+4', 'weighted', 3),
    (32, 8, 'padded16', 'padded16', 'last', 1),
    (32, 8, 'stride+4', 'stride+4', 'first', 3),
    (33, 9, 'tight16', 'pitch+4', 'rank1of3', 1),
    (33, 9, 'offset4', 'stride+4', 'weighted', 3),
    (33, 9, 'pitch+4', 'tight16', 'last', 1),
    (33, 9, 'stride+4', 'offset4', 'first', 3),
    (36, 16, 'tight16', 'pitch+4', 'weighted', 3),
    (36, 16, 'offset4', 'padded16', 'last', 1),
    (36, 16, 'pitch+4', 'stride+4', 'first', 3),
    (36, 16, 'padded16', 'tight16', 'all', 1),
    (36, 16, 'stride+4', 'offset4', 'rank1of3', 3),
    (61, 23, 'tight16', 'tight16', 'last', 1),
    (61, 23, 'offset4', 'offset4', 'first', 3),
    (61, 23, 'pitch+4', 'pitch+4', 'all', 1),
    (61, 23, 'stride+4', 'stride+4', 'rank1of3', 3),
    (64, 61, 'tight16', 'stride+4', 'first', 3),
    (64, 61, 'offset4', 'tight16', 'all', 1),
    (64, 61, 'pitch+4', 'offset4', 'rank1of3', 3),
    (64, 61, 'padded16', 'pitch+4', 'weighted', 1),
    (64, 61, 'stride+4', 'padded16', 'last', 3),
    (100, 7, 'tight16', 'padded16', 'all', 1),
    (100, 7, 'offset4', 'offset4', 'rank1of3', 3),
    (100, 7, 'pitch+4', 'pitch+4', 'weighted', 1),
    (100, 7, 'padded16', 'tight16', 'last', 3),
    (100, 7, 'stride+4', 'stride+4', 'first', 3),
    (333, 61, 'tight16', 'stride+4', 'rank1of3', 3),
    (333, 61, 'offset4', 'tight16', 'weighted', 1),
    (333, 61, 'pitch+4', 'offset4', 'last', 3),
    (333, 61, 'stride+4', 'pitch+4', 'first', 3),
    (32, 23, 'tight16', 'padded16', 'weighted', 1),
    (32, 23, 'offset4', 'padded16', 'last', 3),
    (32, 23, 'pitch+4', 'stride+4', 'first', 3),
    (32, 23, 'padded16', 'tight16', 'all', 3),
    (32, 23, 'stride+4', 'offset4', 'rank1of3', 3),
    (33, 61, 'tight16', 'offset4', 'last', 3),
    (33, 61, 'offset4', 'pitch+4', 'first', 1),
    (33, 61, 'pitch+4', 'stride+4', 'all', 3),
    (33, 61, 'stride+4', 'tight16', 'rank1of3', 3),
    (64, 8, 'tight16', 'padded16', 'first', 1),
    (64, 8, 'offset4', 'tight16', 'all', 3),
    (64, 8, 'pitch+4', 'offset4', 'rank1of3', 1),
    (64, 8, 'padded16', 'tight16', 'weighted', 3),
    (64, 8, 'stride+4', 'padded16', 'last', 3),
    (1, 61, 'tight16', 'stride+4', 'all', 3),
    (1, 61, 'offset4', 'tight16', 'rank1of3', 1),
    (1, 61, 'pitch+4', 'offset4', 'weighted', 3),
    (1, 61, 'stride+4', 'pitch+4', 'last', 3),
    (4, 1, 'tight16', 'padded16', 'rank1of3', 1),
    (4, 1, 'offset4', 'pitch+4', 'weighted', 3),
    (4, 1, 'pitch+4', 'padded16', 'last', 1),
    (4, 1, 'padded16', 'tight16', 'first', 3),
    (4, 1, 'stride+4', 'tight16', 'all', 3),
    (36, 9, 'tight16', 'pitch+4', 'weighted', 3),
    (36, 9, 'offset4', 'padded16', 'last', 1),
    (36, 9, 'pitch+4', 'stride+4', 'first', 3),
    (36, 9, 'padded16', 'tight16', 'all', 1),
    (36, 9, 'stride+4', 'offset4', 'rank1of3', 3),
    (100, 16, 'tight16', 'padded16', 'last', 1),
    (100, 16, 'offset4', 'stride+4', 'first', 3),
    (100, 16, 'pitch+4', 'tight16', 'all', 1),
    (100, 16, 'padded16', 'tight16', 'rank1of3', 3),
    (100, 16, 'stride+4', 'pitch+4', 'weighted', 3),
    (333, 23, 'tight16', 'stride+4', 'first', 3),
    (333, 23, 'offset4', 'tight16', 'all', 1),
    (333, 23, 'pitch+4', 'offset4', 'rank1of3', 3),
    (333, 23, 'stride+4', 'pitch+4', 'weighted', 3),
    (34, 16, 'tight16', 'tight16', 'all', 1),
    (34, 16, 'offset4', 'offset4', 'rank1of3', 3),
    (34, 16, 'pitch+4', 'pitch+4', 'weighted', 1),
    (34, 16, 'stride+4', 'stride+4', 'last', 3),
    (2, 9, 'tight16', 'offset4', 'rank1of3', 3),
    (2, 9, 'offset4', 'pitch+4', 'weighted', 1),
    (2, 9, 'pitch+4', 'stride+4', 'last', 3),
    (2, 9, 'stride+4', 'tight16', 'first', 3),
]
IDS = ["%dx%d-%s-%s-%s-%d" % c for c in CASES]


def layout(name, W, rows):
    """The view of `rows` rows of W pixels per frame inside an allocation whose first byte is 16-byte aligned."""
    if name == "tight16":
        return M.Layout(GUARD, 4 * W, rows * 4 * W)
    if name == "offset4":
        return M.Layout(GUARD + 4, 4 * W, rows * 4 * W)
    if name == "pitch+4":
        return M.Layout(GUARD, 4 * W + 4, rows * (4 * W + 4))
    if name == "padded16":
        assert W % 4 == 0
        pitch = (4 * W + 15) // 16 * 16 + 16
        return M.Layout(GUARD, pitch, rows * pitch + 16)
    if name == "stride+4":
        return M.Layout(GUARD, 4 * W, rows * 4 * W + 4)
    raise KeyError(name)


def alloc_size(lay, count):
    return (lay.base + count * lay.stride + GUARD + 15) // 16 * 16


def aligned16(lay):
    return (lay.base | lay.pitch | lay.stride) & 15 == 0


def stripe_list(kifs, name, H):
    n = (H + 7) // 8
    if name == "all":
        return list(range(n))
    if name == "rank1of3":
        return kifs.shard_stripes(H, 1, 3)[0]
    if name == "weighted":
        return kifs.shard_stripes(H, 1, 3, weights=[1, 2, 1])[0]
    return [n - 1] if name == "last" else [0]


class Case:
    def __init__(self, kifs, index):
        self.index = index
        self.W, self.H, fl, sl, st, self.count = CASES[index]
        self.stripes = stripe_list(kifs, st, self.H)
        self.rows = sum(M.stripe_rows(s, self.H) for s in self.stripes)
        self.fl, self.sl = layout(fl, self.W, self.H), layout(sl, self.W, self.rows)
        self.tiles = self.count * len(self.stripes) * M.tiles_x(self.W)
        # the launchers' own rules, on the layout (the allocations themselves are 16-byte aligned: asserted at upload)
        self.vec16 = {"unpack_stripes": aligned16(self.fl) and aligned16(self.sl) and (4 * self.W) & 15 == 0,
                      "fill_stripes": aligned16(self.fl) and (4 * self.W) & 15 == 0,
                      "pack_sparse": aligned16(self.sl)}

    def tile_kinds(self):
        """(shard, stripe slot, tile column, kind) for every tile: what shard_alloc lays over the random pixels."""
        t = 0
        for i in range(self.count):
            for k in range(len(self.stripes)):
                for c in range(M.tiles_x(self.W)):
                    yield i, k, c, (t + self.index) % 8
                    t += 1

    def shard_alloc(self, bg):
        """The packed shards' allocation: seeded random pixels, and per tile one of
        0 left random; 1 wholly background; background but for one pixel at 2 (row 0, col 0) / 3 (row 7, col 31), clipped
        to the frame / 4 the last in-frame column / 5 the last in-frame row / 6 anywhere, differing in the alpha byte only;
        7 wholly background with non-background garbage in the pitch padding to its right (right-edge tiles of a padded
        pitch: it must not produce a record)."""
        W, lay = self.W, self.sl
        rng = np.random.default_rng(1000 + self.index)
        buf = np.full(alloc_size(lay, self.count), CANARY, dtype=np.uint8)
        for i in range(self.count):
            for r in range(self.rows):
                at = lay.base + i * lay.stride + r * lay.pitch
                buf[at:at + 4 * W] = rng.integers(0, 256, size=4 * W, dtype=np.uint8)
        for i, k, c, kind in self.tile_kinds():
            if kind == 0:
                continue
            rows, w = M.stripe_rows(self.stripes[k], self.H), min(M.TILE_W, W - c * M.TILE_W)
            at = lambda r, x: lay.base + i * lay.stride + (8 * k + r) * lay.pitch + 4 * (c * M.TILE_W + x)
            for r in range(rows):
                M.put_words(buf, at(r, 0), np.full(w, bg, dtype="<u4"))
            pixel = {2: (0, 0, 0x00010000), 3: (rows - 1, w - 1, 0x00000100), 4: (rows // 2, w - 1, 0x00000001),
                     5: (rows - 1, w // 2, 0x00800000), 6: (rows // 2, w // 2, 0x01000000)}.get(kind)
            if pixel:
                M.put_words(buf, at(pixel[0], pixel[1]), np.array([bg ^ pixel[2]], dtype="<u4"))
            if kind == 7 and c == M.tiles_x(W) - 1:
                for r in range(rows):
                    buf[at(r, w):at(r, 0) - 4 * c * M.TILE_W + lay.pitch] = 0x3C
        return buf

    def frame_alloc(self):
        return np.full(alloc_size(self.fl, self.count), CANARY, dtype=np.uint8)

    def record_alloc(self):
        return np.full(2 * GUARD + max(self.tiles, 1) * 1040, CANARY, dtype=np.uint8)


def test_case_table_covers_the_code_paths(kifs):
    """The table is what the issue asks for, by its own count: every W % 4, narrow / exact / just-over-one-tile widths,
    short, whole and ragged heights, every layout for every shape, both values of vec16 for each kernel that has the
    switch (aligned and unaligned frames for unpack_sparse, which has none), and the tile contents that need a ragged
    edge do meet one."""
    assert len(CASES) == 98 and len(set(CASES)) == 98
    shapes = sorted({(c[0], c[1]) for c in CASES})
    assert len(shapes) == 22
    assert {w % 4 for w, _ in shapes} == {0, 1, 2, 3}
    assert any(w < 32 for w, _ in shapes) and any(w == 32 for w, _ in shapes) and any(w == 33 for w, _ in shapes)
    assert any(h < 8 for _, h in shapes) and any(h % 8 == 0 for _, h in shapes) and any(h % 8 for _, h in shapes)
    for w, h in shapes:
        want = {l for l in LAYOUTS if l != "padded16" or w % 4 == 0}
        assert {c[2] for c in CASES if (c[0], c[1]) == (w, h)} == want, (w, h)
    assert {c[3] for c in CASES} == set(LAYOUTS) and {c[4] for c in CASES} == set(STRIPE_LISTS)
    assert {c[5] for c in CASES} == {1, 3}
    assert all(c[5] == 3 for c in CASES if "stride+4" in c[2:4])
    cases = [Case(kifs, i) for i in range(len(CASES))]
    for kernel in ("unpack_stripes", "fill_stripes", "pack_sparse"):
        assert {bool(c.vec16[kernel]) for c in cases} == {True, False}, kernel
    assert {aligned16(c.fl) for c in cases if c.stripes} == {True, False}  # unpack_sparse: frames either way
    # a frame layout that is aligned against a shard layout that is not, and the other way round
    assert any(aligned16(c.fl) and not aligned16(c.sl) and c.W % 4 == 0 for c in cases)
    assert any(aligned16(c.sl) and not aligned16(c.fl) and c.W % 4 == 0 for c in cases)
    seen = set()
    for c in cases:
        for i, k, col, kind in c.tile_kinds():
            ragged_x = col == M.tiles_x(c.W) - 1 and c.W % 32 != 0
            ragged_y = M.stripe_rows(c.stripes[k], c.H) < 8
            seen.add((kind, "any"))
            if ragged_x:
                seen.add((kind, "ragged_x"))
            if ragged_y:
                seen.add((kind, "ragged_y"))
            if kind == 7 and ragged_x and c.sl.pitch > 4 * c.W:
                seen.add((7, "padding"))
            if not ragged_x and not ragged_y:
                seen.add((kind, "whole"))
    for kind in range(8):
        assert {(kind, "any"), (kind, "ragged_x"), (kind, "ragged_y")} <= seen, kind
    assert (7, "padding") in seen and (3, "whole") in seen and (2, "whole") in seen


# ---- the GPU side ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def backgrounds(gs, kifs, oracle):
    """{encode: background pixel} of the options the module's cases run under: a non-grey colour, read off an oracle
    frame whose camera is too far away to see anything."""
    from kifs_raymarching_amd.configs import WORKLOADS
    w = WORKLOADS["cfg2_julia_1080p"]
    gui = dataclasses.replace(w.gui, background_color=(200, 40, 90))
    bg = {}
    for encode in (kifs.ENCODE_UNORM, kifs.ENCODE_SRGB):
        far = oracle_frame(oracle, kifs, kifs.ScreenData(64, 8), kifs.CameraData(origin_distance=50.0), gui, w.iters,
                           encode=encode)
        assert (far == far[0, 0]).all()
        bg[encode] = int(far[0, 0, 0]) | int(far[0, 0, 1]) << 8 | int(far[0, 0, 2]) << 16 | int(far[0, 0, 3]) << 24
    assert bg[0] != bg[1] and len({bg[1] & 255, bg[1] >> 8 & 255, bg[1] >> 16 & 255}) == 3
    return gui, bg


class Device:
    """Uploads, library calls on the context's stream, downloads -- each call complete before the next."""

    def __init__(self, gs, kifs, gui, W, H):
        import torch
        from kifs_raymarching_amd._lib import lib
        self.torch, self.lib, self.gs, self.ctx = torch, lib, gs, gs._ctx
        gs.update_screen_data(kifs.ScreenData(W, H))
        gs.update_options(gui)

    def up(self, host):
        t = self.torch.from_numpy(host.copy()).to("cuda:0")
        self.torch.cuda.synchronize()
        assert t.data_ptr() % 16 == 0
        return t

    def down(self, t):
        self.gs.synchronize()
        return t.cpu().numpy()

    @staticmethod
    def st(stripes):
        return (C.c_int * len(stripes))(*stripes)

    def unpack_shard(self, count, frames, fl, shards, sl, stripes):
        return self.lib.kifs_unpack_shard_async(self.ctx, None, count, frames.data_ptr() + fl.base, fl.pitch, fl.stride,
                                                shards.data_ptr() + sl.base, sl.pitch, sl.stride, self.st(stripes), len(stripes))

    def fill(self, count, frames, fl, stripes, encode):
        return self.lib.kifs_fill_shard_async(self.ctx, None, count, frames.data_ptr() + fl.base, fl.pitch, fl.stride,
                                              self.st(stripes), len(stripes), encode)

    def pack(self, count, shards, sl, stripes, encode, records, capacity, n_dev, n_host, records_at=GUARD):
        return self.lib.kifs_pack_sparse_async(self.ctx, None, count, shards.data_ptr() + sl.base, sl.pitch, sl.stride,
                                               self.st(stripes), len(stripes), encode, records.data_ptr() + records_at,
                                               capacity, n_dev.data_ptr() + 16, n_host.data_ptr())

    def unpack_sparse(self, count, frames, fl, records, n, stripes, erase_encode=None, records_at=GUARD):
        args = (self.ctx, None, count, frames.data_ptr() + fl.base, fl.pitch, fl.stride, records.data_ptr() + records_at, n,
                self.st(stripes), len(stripes))
        if erase_encode is None:
            return self.lib.kifs_unpack_sparse_async(*args)
        return self.lib.kifs_erase_sparse_async(*args, erase_encode)

    def counters(self):
        """(device words around the record counter, pinned host word), both preset to values a pack must overwrite."""
        n_dev = self.up(np.array([0xA5A5A5A5] * 4 + [77] + [0xA5A5A5A5] * 3, dtype=np.uint32).view(np.uint8))
        n_host = self.torch.full((1,), 99, dtype=self.torch.int32).pin_memory()
        return n_dev, n_host


def records_into(alloc, records):
    alloc[GUARD:GUARD + records.size * 4] = records.view(np.uint8).reshape(-1)
    return alloc


@gpu
@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_unpack_shard(index, gs, kifs, backgrounds):
    gui, bg = backgrounds
    c = Case(kifs, index)
    d = Device(gs, kifs, gui, c.W, c.H)
    shards, frames = c.shard_alloc(bg[1]), c.frame_alloc()
    d_shards, d_frames = d.up(shards), d.up(frames)
    assert d.unpack_shard(c.count, d_frames, c.fl, d_shards, c.sl, c.stripes) == 0
    want = M.unpack_stripes(frames.copy(), shards, (c.fl, c.sl), c.stripes, c.W, c.H, c.count)
    got = d.down(d_frames)
    assert (got == want).all(), np.flatnonzero(got != want)[:8]
    assert (d.down(d_shards) == shards).all()


@gpu
@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_fill(index, gs, kifs, backgrounds):
    gui, bg = backgrounds
    c = Case(kifs, index)
    d = Device(gs, kifs, gui, c.W, c.H)
    for encode in (1, 0):
        frames = c.frame_alloc()
        d_frames = d.up(frames)
        assert d.fill(c.count, d_frames, c.fl, c.stripes, encode) == 0
        want = M.fill_stripes(frames.copy(), c.fl, c.stripes, c.W, c.H, c.count, bg[encode])
        got = d.down(d_frames)
        assert (got == want).all(), (encode, np.flatnonzero(got != want)[:8])


@gpu
@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_pack(index, gs, kifs, backgrounds):
    gui, bg = backgrounds
    c = Case(kifs, index)
    d = Device(gs, kifs, gui, c.W, c.H)
    for encode in (1, 0):
        shards = c.shard_alloc(bg[encode])
        want = M.pack_sparse(shards, c.sl, c.stripes, c.W, c.H, c.count, bg[encode])
        d_shards, d_records = d.up(shards), d.up(c.record_alloc())
        n_dev, n_host = d.counters()
        assert d.pack(c.count, d_shards, c.sl, c.stripes, encode, d_records, c.tiles, n_dev, n_host) == 0
        words = d.down(n_dev).view(np.uint32)
        n = int(words[4])
        assert n == int(n_host[0]) == len(want), (encode, n, int(n_host[0]), len(want))
        assert (words[:4] == 0xA5A5A5A5).all() and (words[5:] == 0xA5A5A5A5).all()
        raw = d.down(d_records)
        got = raw[GUARD:GUARD + n * 1040].view(np.uint32).reshape(n, M.RECORD_WORDS)
        assert len(np.unique(got[:, 0])) == n and not got[:, 1:4].any(), encode
        got = got[np.argsort(got[:, 0], kind="stable")]
        assert (got == want).all(), (encode, np.argwhere(got != want)[:8])
        assert (raw[:GUARD] == CANARY).all() and (raw[GUARD + n * 1040:] == CANARY).all(), encode
        assert (d.down(d_shards) == shards).all()


@gpu
@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_unpack_sparse_and_erase(index, gs, kifs, backgrounds):
    gui, bg = backgrounds
    c = Case(kifs, index)
    d = Device(gs, kifs, gui, c.W, c.H)
    records = M.pack_sparse(c.shard_alloc(bg[1]), c.sl, c.stripes, c.W, c.H, c.count, bg[1])
    rng = np.random.default_rng(2000 + index)
    records = records[rng.permutation(len(records))]  # the payload's order is arbitrary
    foreign = np.full((2, M.RECORD_WORDS), 0x5A5A5A5A, dtype="<u4")
    foreign[:, 1:4] = 0
    foreign[0, 0], foreign[1, 0] = c.tiles, 0xffffffff  # the first id out of range, and the largest
    room = max(c.tiles - 2, 0)                          # (a call takes at most one record per tile)
    spliced = np.concatenate([records[:room][:1], foreign[:1], records[:room][1:], foreign[1:]])[:c.tiles]
    for recs, encode in ((records, 1), (spliced, 0)):
        frames = c.frame_alloc()
        d_frames, d_records = d.up(frames), d.up(records_into(c.record_alloc(), recs))
        assert d.unpack_sparse(c.count, d_frames, c.fl, d_records, len(recs), c.stripes) == 0
        want = M.unpack_sparse(frames.copy(), c.fl, recs, c.stripes, c.W, c.H, c.count)
        got = d.down(d_frames)
        assert (got == want).all(), ("unpack", encode, np.flatnonzero(got != want)[:8])
        assert d.unpack_sparse(c.count, d_frames, c.fl, d_records, len(recs), c.stripes, erase_encode=encode) == 0
        want = M.unpack_sparse(want, c.fl, recs, c.stripes, c.W, c.H, c.count, erase=True, bg=bg[encode])
        got = d.down(d_frames)
        assert (got == want).all(), ("erase", encode, np.flatnonzero(got != want)[:8])
        assert (d.down(d_records) == records_into(c.record_alloc(), recs)).all()


@gpu
@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_round_trip(index, gs, kifs, backgrounds):
    """fill + unpack_sparse(pack(shards)) == unpack_shard(shards) on the listed rows, all on the device."""
    gui, bg = backgrounds
    c = Case(kifs, index)
    d = Device(gs, kifs, gui, c.W, c.H)
    d_shards = d.up(c.shard_alloc(bg[1]))
    d_records = d.up(c.record_alloc())
    n_dev, n_host = d.counters()
    sparse, dense = d.up(c.frame_alloc()), d.up(c.frame_alloc())
    assert d.fill(c.count, sparse, c.fl, c.stripes, 1) == 0
    assert d.pack(c.count, d_shards, c.sl, c.stripes, 1, d_records, c.tiles, n_dev, n_host) == 0
    gs.synchronize()
    assert d.unpack_sparse(c.count, sparse, c.fl, d_records, int(n_host[0]), c.stripes) == 0
    assert d.unpack_shard(c.count, dense, c.fl, d_shards, c.sl, c.stripes) == 0
    sparse, dense = d.down(sparse), d.down(dense)
    listed = np.zeros(sparse.size, dtype=bool)
    for i in range(c.count):
        for s in c.stripes:
            for r in range(M.stripe_rows(s, c.H)):
                at = c.fl.base + i * c.fl.stride + (8 * s + r) * c.fl.pitch
                listed[at:at + 4 * c.W] = True
    assert int(listed.sum()) == c.count * c.rows * 4 * c.W
    assert (sparse[listed] == dense[listed]).all()
    assert (sparse[~listed] == CANARY).all() and (dense[~listed] == CANARY).all()


@gpu
def test_argument_checks_through_the_abi(gs, kifs, backgrounds):
    """What the header requires of pitches, strides and pointers: a violation is KIFS_ERR_BAD_SIZE and nothing is written."""
    gui, bg = backgrounds
    W, H, count, stripes = 36, 16, 3, [0, 1]
    d = Device(gs, kifs, gui, W, H)
    ok = M.Layout(GUARD, 4 * W + 16, H * (4 * W + 16) + 16)
    frames = np.full(alloc_size(ok, count) + 64, CANARY, dtype=np.uint8)
    shards = np.random.default_rng(5).integers(0, 256, size=frames.size, dtype=np.uint8)
    records = np.full(2 * GUARD + 13 * 1040, CANARY, dtype=np.uint8)  # (room for every tile, whatever runs)
    records[GUARD:GUARD + 4] = 0  # a valid record 0 should a bad call run after all
    d_frames, d_shards, d_records = d.up(frames), d.up(shards), d.up(records)
    n_dev, n_host = d.counters()
    tiles = count * len(stripes) * 2
    bad = [ok._replace(pitch=4 * W - 4), ok._replace(pitch=4 * W + 2), ok._replace(stride=ok.stride + 2),
           ok._replace(base=GUARD + 2)]
    for lay in bad:
        assert d.unpack_shard(count, d_frames, lay, d_shards, ok, stripes) == BAD_SIZE, lay
        assert d.unpack_shard(count, d_frames, ok, d_shards, lay, stripes) == BAD_SIZE, lay
        assert d.fill(count, d_frames, lay, stripes, 1) == BAD_SIZE, lay
        assert d.pack(count, d_shards, lay, stripes, 1, d_records, tiles, n_dev, n_host) == BAD_SIZE, lay
        assert d.unpack_sparse(count, d_frames, lay, d_records, 1, stripes) == BAD_SIZE, lay
        assert d.unpack_sparse(count, d_frames, lay, d_records, 1, stripes, erase_encode=1) == BAD_SIZE, lay
    assert d.pack(count, d_shards, ok, stripes, 1, d_records, tiles, n_dev, n_host, records_at=GUARD + 8) == BAD_SIZE
    assert d.pack(count, d_shards, ok, stripes, 1, d_records, tiles - 1, n_dev, n_host) == BAD_SIZE
    assert d.unpack_sparse(count, d_frames, ok, d_records, 1, stripes, records_at=GUARD + 8) == BAD_SIZE
    assert d.unpack_sparse(count, d_frames, ok, d_records, 1, stripes, erase_encode=1, records_at=GUARD + 8) == BAD_SIZE
    assert d.unpack_sparse(count, d_frames, ok, d_records, tiles + 1, stripes) == BAD_SIZE
    assert (d.down(d_frames) == frames).all() and (d.down(d_shards) == shards).all()
    assert (d.down(d_records) == records).all()
    assert int(d.down(n_dev).view(np.uint32)[4]) == 77 and int(n_host[0]) == 99


@gpu
def test_shard_count_beyond_the_grid_limit(gs, kifs, backgrounds):
    """The shard index is one dimension of the launch grid: KIFS_MAX_SHARD_COUNT = 65535 shards are copied and filled,
    65536 are refused with KIFS_ERR_BAD_SIZE before anything is written (1 x 8 frames: 2 MiB a buffer)."""
    gui, bg = backgrounds
    W, H, count = 1, 8, 65536
    d = Device(gs, kifs, gui, W, H)
    lay = M.Layout(GUARD, 4, 32)
    frames = np.full(alloc_size(lay, count), CANARY, dtype=np.uint8)
    shards = np.random.default_rng(9).integers(0, 256, size=frames.size, dtype=np.uint8)
    d_frames, d_shards = d.up(frames), d.up(shards)
    assert d.unpack_shard(count, d_frames, lay, d_shards, lay, [0]) == BAD_SIZE
    assert d.fill(count, d_frames, lay, [0], 1) == BAD_SIZE
    assert (d.down(d_frames) == frames).all()
    assert d.unpack_shard(count - 1, d_frames, lay, d_shards, lay, [0]) == 0
    want = frames.copy()
    want[GUARD:GUARD + 32 * (count - 1)] = shards[GUARD:GUARD + 32 * (count - 1)]
    assert (d.down(d_frames) == want).all()
    assert d.fill(count - 1, d_frames, lay, [0], 1) == 0
    want[GUARD:GUARD + 32 * (count - 1)] = np.tile(np.array([bg[1]], dtype="<u4").view(np.uint8), 8 * (count - 1))
    assert (d.down(d_frames) == want).all()


# ---- the tile order on chosen costs ----------------------------------------------------------------------------
# (n, tiles_x): 1 .. 65 straddle a wave, 1023 .. 1025 a round of the 1024-thread workgroup, 8100 is a 1080p frame,
# 129 600 an 8K one (127 rounds).  (129600, 1) would be 129 600 tile rows: refused, see test_sort_tiles_argument_checks.
SORT_SHAPES = [(1, 1), (1, 60), (1, 240), (63, 1), (63, 60), (63, 240), (64, 1), (64, 60), (64, 240), (65, 1), (65, 60),
               (65, 240), (1023, 1), (1023, 60), (1023, 240), (1024, 1), (1024, 60), (1024, 240), (1025, 1), (1025, 60),
               (1025, 240), (8100, 1), (8100, 60), (8100, 240), (129600, 60), (129600, 240)]


def cost_tables(n):
    """(name, costs, shift)."""
    rng = np.random.default_rng(n)
    z = np.zeros(n, dtype=np.uint32)
    one_last, one_first, sparse = z.copy(), z.copy(), z.copy()
    one_last[n - 1], one_first[0] = 5, 700
    live = rng.random(n) < 0.02
    sparse[live] = rng.integers(1, 4000, size=int(live.sum()), dtype=np.uint32)
    dense = rng.integers(0, 2 ** 32, size=n, dtype=np.uint32)
    ramp = np.arange(n, dtype=np.uint32)
    return [("zero", z, 0), ("equal", np.full(n, 300, dtype=np.uint32), 0), ("saturated", np.full(n, 0xffffffff, dtype=np.uint32), 0),
            ("one_last", one_last, 0), ("one_first", one_first, 0), ("sparse", sparse, 0), ("sparse_shift", sparse, 2),
            ("dense0", dense, 0), ("dense5", dense, 5), ("dense31", dense, 31), ("dense22", dense, 22),
            ("ramp", ramp, max(0, int(n - 1).bit_length() - 10))]


@gpu
@pytest.mark.parametrize("n,tiles_x", SORT_SHAPES)
def test_tile_order_is_a_sorted_permutation(n, tiles_x, gs):
    """tile_order_kernel's promise -- a permutation whatever the costs hold, heaviest bin first -- on chosen costs."""
    ids = np.sort(M.tile_ids(n, tiles_x))
    for name, cost, shift in cost_tables(n):
        bins = M.tile_bins(cost, shift)
        if name == "ramp":
            assert len(np.unique(bins)) >= min(n, 500), "the ramp spreads over the bins"
        sequences = []
        for _ in range(2):
            before = cost.copy()
            order, after = gs.debug_sort_tiles(cost, tiles_x, shift)
            assert (cost == before).all()
            assert order.shape == (n,) and (np.sort(order) == ids).all(), (name, "not a permutation of the tiles")
            index = (order & 0xffff).astype(np.int64) + (order >> 16).astype(np.int64) * tiles_x
            sequences.append(bins[index])
            assert (np.diff(sequences[-1]) >= 0).all(), (name, "heavier tiles do not come first")
            assert not after.any(), (name, "the cost table is not left zeroed")
        assert (sequences[0] == sequences[1]).all(), name


@gpu
def test_sort_tiles_argument_checks(gs):
    from kifs_raymarching_amd._lib import lib
    cost = np.arange(70000, dtype=np.uint32)
    order, after = np.full(70000, 7, dtype=np.uint32), np.full(70000, 9, dtype=np.uint32)
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    for n, tiles_x, shift in ((0, 1, 0), (8, 0, 0), (8, 65537, 0), (65537, 1, 0), (70000, 1, 0), (8, 4, 32)):
        assert lib.kifs_debug_sort_tiles(gs._ctx, up(cost), n, tiles_x, shift, up(order), up(after)) in (BAD_SIZE, BAD_ARG)
    assert lib.kifs_debug_sort_tiles(gs._ctx, None, 8, 4, 0, up(order), up(after)) == BAD_ARG
    assert lib.kifs_debug_sort_tiles(gs._ctx, up(cost), 8, 4, 0, None, up(after)) == BAD_ARG
    assert lib.kifs_debug_sort_tiles(gs._ctx, up(cost), 8, 4, 0, up(order), None) == BAD_ARG
    assert (order == 7).all() and (after == 9).all() and (cost == np.arange(70000)).all()
    # the limits themselves are accepted: 65536 columns, 65536 rows
    o, a = gs.debug_sort_tiles(cost[:65536], 65536, 3)
    assert (np.sort(o) == np.arange(65536)).all() and not a.any()
    o, a = gs.debug_sort_tiles(cost[:65536], 1, 31)
    assert (np.sort(o) == np.arange(65536, dtype=np.uint32) << 16).all() and not a.any()


@gpu
def test_sort_tiles_leaves_the_contexts_own_order_alone(gs, kifs):
    gs.update_screen_data(kifs.ScreenData(333, 61))
    before = gs.debug_get_tile_order()
    gs.debug_sort_tiles(np.arange(before.size, dtype=np.uint32)[::-1], 11, 0)
    assert (gs.debug_get_tile_order() == before).all()
