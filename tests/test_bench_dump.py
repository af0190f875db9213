"""bench.py --dump-outputs, as far as a box without a GPU can show it: dump_outputs() writes the frames it is given as
float32 .npy files -- all of them when they fit in 64 MB, else a fixed sample of their pixels with each pixel's
(frame, row, column) -- and the same frames give the same files.  (The GPU half, bench.py's own runs, is in
tests/test_gpu_bench.py.)"""
import numpy as np
import torch

import bench


def test_small_frames_are_written_whole(tmp_path):
    frames = torch.randint(0, 256, (3, 8, 16, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    assert bench.dump_outputs(tmp_path, frames) == ["frames.npy"]
    got = np.load(tmp_path / "frames.npy")
    assert got.dtype == np.float32 and np.array_equal(got, frames.numpy().astype(np.float32))


def test_large_frames_are_sampled_the_same_way_every_time(tmp_path):
    n, H, W = 9, 1080, 1920  # 9 x 1080p RGBA as float32: 299 MB, over the budget
    frames = torch.randint(0, 256, (n, H, W, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(2))
    for d in ("a", "b"):
        assert bench.dump_outputs(tmp_path / d, frames) == ["frames_sample.npy", "frames_sample_at.npy"]
        assert sum(f.stat().st_size for f in (tmp_path / d).iterdir()) <= bench.DUMP_BUDGET_BYTES
    rgba, at = np.load(tmp_path / "a" / "frames_sample.npy"), np.load(tmp_path / "a" / "frames_sample_at.npy")
    assert rgba.dtype == at.dtype == np.float32 and rgba.shape[1] == 4 and at.shape == (rgba.shape[0], 3)
    assert 0.9 * bench.DUMP_SAMPLE_PIXELS < rgba.shape[0] <= bench.DUMP_SAMPLE_PIXELS
    assert np.array_equal(rgba, np.load(tmp_path / "b" / "frames_sample.npy"))
    assert np.array_equal(at, np.load(tmp_path / "b" / "frames_sample_at.npy"))
    f, y, x = (at[:, i].astype(np.int64) for i in range(3))
    assert f.max() == n - 1 and y.max() == H - 1 and x.max() == W - 1 and len(set(zip(f, y, x))) == len(f)
    assert np.array_equal(rgba, frames.numpy()[f, y, x].astype(np.float32))
