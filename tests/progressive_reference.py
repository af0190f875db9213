"""The expected frames AND plane of progressive accumulation (include/kifs_hip.h, kifs_render_accumulate_resume_async),
from the unmodified oracle.  The model literally carries a plane between passes, as the contract words it: a pass over
the (count, samples, H, W, 3) linear sub-frames of its views (jitter_reference.linear_views: the oracle's colour of every
view at its cell's pixel of the virtual screen) starts from c_0 when the plane holds nothing (prior == 0: the plane is
not read) or from the plane's sum, adds the sub-frames in order in np.float32, and leaves (acc, np.float32(total)) in the
plane; the picture is aa_reference.encode (the oracle's encoder) of acc / np.float32(total).  Nothing here knows that
the fold is associative with the one-call model (accumulate_reference.resolve): tests/test_progressive_reference.py
shows that it is."""
import numpy as np

import aa_reference as AA
import jitter_reference as JR


def fold(plane, prior, lin):
    """One pass.  `plane`: (count, H, W, 4) float32 or None (allowed with prior == 0); `lin`: (count, samples, H, W, 3)
    float32 linear sub-frames.  Returns the new plane (a new array) and the new total."""
    lin = np.asarray(lin, dtype=np.float32)
    count, samples = lin.shape[:2]
    if prior == 0:
        acc = lin[:, 0].astype(np.float32).copy()
        first = 1
    else:
        acc = np.asarray(plane, dtype=np.float32)[..., :3].copy()
        first = 0
    for s in range(first, samples):
        acc = (acc + lin[:, s]).astype(np.float32)
    total = prior + samples
    out = np.empty(lin.shape[:1] + lin.shape[2:4] + (4,), dtype=np.float32)
    out[..., :3] = acc
    out[..., 3] = np.float32(total)
    return out, total


def picture(O, plane, encode_mode=1):
    """(count, H, W, 4) uint8: encode(sum / float(total)) of every frame of a plane."""
    mean = (plane[..., :3] / plane[..., 3:]).astype(np.float32)
    return np.stack([AA.encode(O, m, encode_mode) for m in mean])


def split_views(lin, count, samples, splits):
    """(count * samples, H, W, 3) sub-frames of ONE call -> per pass the (count, n, H, W, 3) sub-frames of its views:
    pass p holds sub-frames [sum(splits[:p]), sum(splits[:p + 1])) of every frame."""
    assert sum(splits) == samples and lin.shape[0] == count * samples
    groups = lin.reshape(count, samples, *lin.shape[1:])
    out, done = [], 0
    for n in splits:
        out.append(groups[:, done:done + n])
        done += n
    return out


def pass_views(items, count, samples, splits):
    """The same regrouping for per-view lists of a one-call launch (cameras, options, cells): per pass the list of its
    count * n views in the call's order (frame-major)."""
    assert len(items) == count * samples and sum(splits) == samples
    out, done = [], 0
    for n in splits:
        out.append([items[f * samples + done + s] for f in range(count) for s in range(n)])
        done += n
    return out


def carried(O, passes, encode_mode=1, y0=0, y1=None, plane=None, prior=0):
    """Runs `passes` (a list of (count, n, H, W, 3) linear sub-frames) one after another through fold().  Returns
    (frames after every pass: list of (count, rows, W, 4) uint8, the final plane's rows (count, rows, W, 4) float32, the
    total)."""
    frames = []
    for lin in passes:
        plane, prior = fold(plane, prior, lin)
        frames.append(picture(O, plane[:, y0:y1], encode_mode))
    return frames, plane[:, y0:y1], prior


def progressive_frames(O, K, screen, cameras, options, iters, samples, g, splits, cells=None, encode_mode=1, lin=None, ext=None,
                       y0=0, y1=None):
    """The one-call arguments of jitter_reference.jittered_frames, rendered as passes of `splits` sub-frames per frame:
    (the final frames, the final plane, the frames after every pass)."""
    if lin is None:
        lin = JR.linear_views(O, K, screen, cameras, options, iters, g, cells, samples, ext)
    count = lin.shape[0] // samples
    frames, plane, total = carried(O, split_views(lin, count, samples, splits), encode_mode, y0, y1)
    assert total == samples
    return frames[-1], plane, frames
