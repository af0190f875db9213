"""The model of progressive accumulation (tests/progressive_reference.py) held to the one-call model on the CPU, so that
tests/test_gpu_progressive.py cannot pass vacuously: for three splits of six sub-frames per frame (2 + 3 + 1, six lone
sub-frames, one pass of 6) the carried plane gives the bytes of jitter_reference.jittered_frames over the concatenated
views, and its sums are accumulate_reference.resolve's accumulator bit for bit; the oracle alone shows that the cases
say something -- the final frame differs from every pass's own frame, and it has pixels every sub-frame hits, pixels
every sub-frame misses and pixels only some hit; and configs.pass_splits is its definition."""
import numpy as np
import pytest

import accumulate_cases as AC
import accumulate_reference as AR
import jitter_reference as JR
import progressive_reference as PR

W, H = 42, 21  # ten columns past a tile edge, five rows past two: small, the oracle runs on the CPU
CELLS = [(0, 0), (2, 2), (1, 0), (2, 0), (0, 2), (1, 1), (2, 1), (0, 1), (1, 2), (1, 1), (0, 0), (2, 2)]  # 2 x 6, g = 3
SPLITS = [(2, 3, 1), (1, 1, 1, 1, 1, 1), (6,)]


@pytest.fixture(scope="module")
def case(oracle, kifs):
    screen, cam, gui, iters = AC.scene(kifs, "julia_24", W, H)
    cams = AC.blur_cameras(kifs, cam, 2, 6)
    lin = JR.linear_views(oracle, kifs, screen, cams, gui, iters, 3, CELLS, 6)
    return screen, cams, gui, iters, lin


def _sums_of_one_call(lin, samples):
    """accumulate_reference.resolve's accumulator before the divide, recomputed the same way."""
    groups = lin.reshape(lin.shape[0] // samples, samples, *lin.shape[1:])
    acc = groups[:, 0].astype(np.float32).copy()
    for s in range(1, samples):
        acc = (acc + groups[:, s]).astype(np.float32)
    return acc


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("encode", [1, 0])
def test_the_carried_model_is_the_one_call_model(splits, encode, case, oracle, kifs):
    screen, cams, gui, iters, lin = case
    want = JR.jittered_frames(oracle, kifs, screen, cams, gui, iters, 6, 3, CELLS, encode, lin=lin)
    got, plane, _ = PR.progressive_frames(oracle, kifs, screen, cams, gui, iters, 6, 3, splits, CELLS, encode, lin=lin)
    assert got.shape == want.shape == (2, H, W, 4) and (got == want).all()
    assert plane.shape == (2, H, W, 4) and plane.dtype == np.float32
    assert (plane[..., :3].view(np.uint32) == _sums_of_one_call(lin, 6).view(np.uint32)).all()
    assert (plane[..., 3] == np.float32(6.0)).all()
    # and the mean the plane describes is resolve's
    mean = (plane[..., :3] / plane[..., 3:]).astype(np.float32)
    assert (mean.view(np.uint32) == AR.resolve(lin, 6).view(np.uint32)).all()


def test_the_cases_are_not_vacuous(case, oracle, kifs):
    screen, cams, gui, iters, lin = case
    final, plane, after = PR.progressive_frames(oracle, kifs, screen, cams, gui, iters, 6, 3, (2, 3, 1), CELLS, lin=lin)
    assert len(after) == 3 and (after[-1] == final).all()
    own = [PR.carried(oracle, [p])[0][0] for p in PR.split_views(lin, 2, 6, (2, 3, 1))]  # every pass on its own
    for frame in own + after[:-1]:
        assert (frame != final).any()
    bg = np.array(list(AC.image(kifs, gui).background_color), dtype=np.float32)
    hits = (lin.reshape(2, 6, H, W, 3) != bg).any(-1).sum(1)  # sub-frames that hit, per frame and pixel
    for f in range(2):
        assert (hits[f] == 6).any() and (hits[f] == 0).any() and ((hits[f] > 0) & (hits[f] < 6)).any()
    # a resumed pass really starts from the plane: another plane, other sums
    passes = PR.split_views(lin, 2, 6, (2, 3, 1))
    first, total = PR.fold(None, 0, passes[0])
    other, _ = PR.fold(first + np.float32(1.0), total, passes[1])
    straight, _ = PR.fold(first, total, passes[1])
    assert (other[..., :3] != straight[..., :3]).any()
    # and a first pass does not read it
    nan = np.full_like(first, np.nan)
    assert (PR.fold(nan, 0, passes[0])[0].view(np.uint32) == first.view(np.uint32)).all()


def test_pass_views_regroups_per_view_lists():
    items = list(range(12))  # 2 frames x 6
    assert PR.pass_views(items, 2, 6, (2, 3, 1)) == [[0, 1, 6, 7], [2, 3, 4, 8, 9, 10], [5, 11]]
    assert PR.pass_views(items, 2, 6, (6,)) == [items]


def test_pass_splits(kifs):
    from kifs_raymarching_amd.configs import pass_splits
    assert pass_splits(150) == [64, 64, 22] and pass_splits(64) == [64] and pass_splits(65) == [64, 1] and pass_splits(1) == [1]
    assert pass_splits(6, 2) == [2, 2, 2] and pass_splits(7, 3) == [3, 3, 1]
    for total in (1, 5, 63, 64, 128, 129, 1000):
        for per in (1, 7, 64):
            got = pass_splits(total, per)
            assert sum(got) == total and all(n == per for n in got[:-1]) and 1 <= got[-1] <= per
            assert len(got) == -(-total // per)
    for bad in ((0, 64), (5, 0), (5, 65), (-1, 4)):
        with pytest.raises(ValueError):
            pass_splits(*bad)


def test_pass_by_pass_cells_concatenate_to_the_one_call_cells(kifs):
    """What tools/render.py --spp and the viewer's refinement hand out: pass p of S sub-frames takes
    jitter_cells(g, S, k + done).  Up to g^2 sub-frames in all the passes' cells concatenate to jitter_cells(g, N, k); beyond
    g^2, to that formula -- n_s = ((s + k) a) mod g^2 -- continued round the grid."""
    from kifs_raymarching_amd.configs import jitter_cells, jitter_stride, pass_splits
    for g in (1, 2, 3, 4, 8):
        n, a = g * g, jitter_stride(g)
        for k in (0, 1, 5):
            for per_pass in {1, min(2, n), min(4, n), n}:  # tools/render.py: at most g^2 per pass
                for N in sorted({1, per_pass, n - 1, n, n + 1, 2 * n + 3, 3 * n} - {0}):
                    got, done = [], 0
                    for S in pass_splits(N, per_pass):
                        got += jitter_cells(g, S, k + done)
                        done += S
                    want = [((((s + k) * a) % n) % g, (((s + k) * a) % n) // g) for s in range(N)]
                    assert got == want, (g, k, per_pass, N)
                    if N <= n:
                        assert got == jitter_cells(g, N, k) and len(set(got)) == N
                    else:
                        assert got[:n] == jitter_cells(g, n, k) and got[n:] == (got[:n] * (N // n + 1))[:N - n]  # round the grid again
