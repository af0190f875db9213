"""tests/support_models.py (the NumPy models the GPU matrix in test_gpu_support_kernels.py compares the kernels with)
against the product's CPU forms in bands.py -- pack_sparse_torch, unpack_sparse_torch, erase_sparse_torch,
fill_stripes_torch, unpack_shards_torch -- on tight layouts at ragged sizes.  The two were written separately, from
include/kifs_hip.h; agreeing byte for byte pins both without a GPU.  Then the models' own handling of what the torch
forms cannot express: offsets, pitch padding, gaps between frames and guard bytes stay exactly as they were."""
import numpy as np
import pytest

import support_models as M

BG = 0xFF30A0E1  # a non-grey background pixel, alpha 255
SIZES = [(1, 1), (3, 7), (5, 9), (31, 8), (33, 23), (61, 61), (64, 16), (100, 23), (333, 61)]


def _stripe_lists(H):
    all_ = list(range((H + 7) // 8))
    return [all_, all_[1::3], all_[-1:], all_[:1], all_[::2]]


def _shards(rng, count, rows, W):
    """Random pixels, about half of the 32 x 8 tiles wholly background, a few pixels differing in alpha only."""
    px = rng.integers(0, 2 ** 32, size=(count, rows, W), dtype=np.uint32)
    for i in range(count):
        for y in range(0, rows, 8):
            for x in range(0, W, 32):
                kind = rng.integers(0, 4)
                if kind >= 2:
                    px[i, y:y + 8, x:x + 32] = BG
                if kind == 3:
                    px[i, min(rows - 1, y + int(rng.integers(0, 8))), min(W - 1, x + int(rng.integers(0, 32)))] = BG ^ 0x01000000
    return px


@pytest.mark.parametrize("size", SIZES)
def test_models_equal_the_cpu_forms_on_tight_layouts(size, kifs):
    import torch
    from kifs_raymarching_amd import bands
    W, H = size
    rng = np.random.default_rng(W * 1000 + H)
    for stripes in _stripe_lists(H):
        rows = sum(M.stripe_rows(s, H) for s in stripes)
        for count in (1, 3):
            px = _shards(rng, count, rows, W)
            flat = px.view(np.uint8).reshape(-1).copy()
            sl = M.Layout(0, 4 * W, rows * 4 * W)
            fl = M.Layout(0, 4 * W, H * 4 * W)
            t_shards = torch.from_numpy(px.view(np.uint8).reshape(count, rows, W, 4).copy())
            # pack
            want = bands.pack_sparse_torch(t_shards, stripes, H, BG).numpy()
            got = M.pack_sparse(flat, sl, stripes, W, H, count, BG)
            assert got.shape[0] == want.shape[0] and (got.view(np.uint8).reshape(-1, 1040) == want).all(), (size, stripes, count)
            assert (np.diff(got[:, 0].astype(np.int64)) > 0).all() and not got[:, 1:4].any()
            # fill + unpack-sparse == dense unpack == the torch forms; then erase
            t_frames = torch.from_numpy(rng.integers(0, 256, size=(count, H, W, 4), dtype=np.uint8))
            frames = t_frames.numpy().reshape(-1).copy()
            dense = frames.copy()
            bands.fill_stripes_torch(t_frames, stripes, BG)
            M.fill_stripes(frames, fl, stripes, W, H, count, BG)
            assert (frames == t_frames.numpy().reshape(-1)).all(), (size, stripes, count)
            foreign = np.zeros((2, M.RECORD_WORDS), dtype="<u4")
            foreign[0, 0], foreign[1, 0] = count * len(stripes) * M.tiles_x(W), 0xffffffff
            foreign[:, 4:] = 0x12345678
            spliced = np.concatenate([got[:1], foreign[:1], got[1:], foreign[1:]])
            bands.unpack_sparse_torch(t_frames, torch.from_numpy(spliced.view(np.uint8).reshape(-1, 1040).copy()), stripes)
            M.unpack_sparse(frames, fl, spliced, stripes, W, H, count)
            assert (frames == t_frames.numpy().reshape(-1)).all(), (size, stripes, count)
            if rows:
                bands.unpack_shards_torch(torch.from_numpy(dense).view(count, H, W, 4), t_shards, stripes)
            assert (M.unpack_stripes(dense.copy(), flat, (fl, sl), stripes, W, H, count) == dense).all()
            ys = [8 * s + r for s in stripes for r in range(M.stripe_rows(s, H))]
            assert (frames.reshape(count, H, W * 4)[:, ys] == dense.reshape(count, H, W * 4)[:, ys]).all()
            bands.erase_sparse_torch(t_frames, torch.from_numpy(spliced.view(np.uint8).reshape(-1, 1040).copy()), stripes, BG)
            M.unpack_sparse(frames, fl, spliced, stripes, W, H, count, erase=True, bg=BG)
            assert (frames == t_frames.numpy().reshape(-1)).all(), (size, stripes, count)


@pytest.mark.parametrize("size", [(5, 9), (36, 23), (33, 8)])
def test_models_touch_only_the_bytes_the_contract_names(size):
    """A layout with an offset, pitch padding and a gap between frames: the model's result, read back through the
    layout, equals the tight result, and every other byte of the allocation is still the canary."""
    W, H = size
    rng = np.random.default_rng(7 * W + H)
    stripes = list(range((H + 7) // 8))[::2]
    rows, count = sum(M.stripe_rows(s, H) for s in stripes), 3
    tight_s, tight_f = M.Layout(0, 4 * W, rows * 4 * W), M.Layout(0, 4 * W, H * 4 * W)
    loose_s = M.Layout(260, 4 * W + 12, rows * (4 * W + 12) + 20)
    loose_f = M.Layout(276, 4 * W + 8, H * (4 * W + 8) + 4)

    def place(tight, n_rows, lay):
        buf = np.full(lay.base + count * lay.stride + 300, 0xA5, dtype=np.uint8)
        mask = np.zeros(buf.size, dtype=bool)
        for i in range(count):
            for r in range(n_rows):
                at = lay.base + i * lay.stride + r * lay.pitch
                buf[at:at + 4 * W] = tight[(i * n_rows + r) * 4 * W:(i * n_rows + r + 1) * 4 * W]
                mask[at:at + 4 * W] = True
        return buf, mask

    px = _shards(rng, count, rows, W).view(np.uint8).reshape(-1)
    shards, _ = place(px, rows, loose_s)
    recs = M.pack_sparse(shards, loose_s, stripes, W, H, count, BG)
    assert (recs == M.pack_sparse(px, tight_s, stripes, W, H, count, BG)).all() and len(recs) > 0
    before = rng.integers(0, 256, size=count * H * W * 4, dtype=np.uint8)
    for op in (lambda f, l: M.fill_stripes(f, l, stripes, W, H, count, BG),
               lambda f, l: M.unpack_sparse(f, l, recs, stripes, W, H, count),
               lambda f, l: M.unpack_sparse(f, l, recs, stripes, W, H, count, erase=True, bg=BG),
               lambda f, l: M.unpack_stripes(f, shards if l is loose_f else px, (l, loose_s if l is loose_f else tight_s),
                                             stripes, W, H, count)):
        want = op(before.copy(), tight_f)
        buf, mask = place(before, H, loose_f)
        got = op(buf, loose_f)
        assert (got[mask] == want).all() and (got[~mask] == 0xA5).all()


def test_tile_bins_and_ids():
    cost = np.array([0, 1, 1022, 1023, 1024, 0xffffffff, 32, 31], dtype=np.uint32)
    assert M.tile_bins(cost, 0).tolist() == [1023, 1022, 1, 0, 0, 0, 991, 992]
    assert M.tile_bins(cost, 5).tolist() == [1023, 1023, 992, 992, 991, 0, 1022, 1023]
    assert M.tile_bins(cost, 31).tolist() == [1023] * 5 + [1022, 1023, 1023]
    assert M.tile_ids(5, 2).tolist() == [0, 1, 0x10000, 0x10001, 0x20000]
    assert M.tile_ids(3, 240).tolist() == [0, 1, 2]
