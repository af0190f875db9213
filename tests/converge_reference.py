"""The expected planes, pictures and counts of converging accumulation (include/kifs_hip.h,
kifs_render_accumulate_converge_async), from the unmodified oracle.  The model carries BOTH planes literally in
np.float32, as the contract words it: the sums plane (sum.r, sum.g, sum.b, n) with n the pixel's own count, and the
moments plane q = the sum of the squared luminances of the pixel's sub-frames.  A pass over the (count, samples, H, W, 3)
linear sub-frames of its views (jitter_reference.linear_views) evaluates `active` on the state the planes hold with the
pass's own rule, folds every active pixel's sub-frames in order, leaves every other pixel's two texels as they are, and
counts the pixels still active afterwards.  It knows no shortcut: every pixel is folded, then the inactive ones are put
back.  The rule is stated once here, as once in the header."""
import numpy as np

import aa_reference as AA

F = np.float32
LIMIT = F(16777216.0)  # 2^24


def luminance(c):
    """Y(c) = (0.2126f*c.r + 0.7152f*c.g) + 0.0722f*c.b in f32, no fma."""
    c = np.asarray(c, dtype=F)
    return ((F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]).astype(F) + (F(0.0722) * c[..., 2]).astype(F)).astype(F)


def tol2(tolerance):
    """tolerance * tolerance: one f32 multiply."""
    with np.errstate(over="ignore"):
        return F(F(tolerance) * F(tolerance))


def active(sums, moments, rule, samples):
    """(count, H, W) bool: active(p) on the state of the planes, with rule = (tolerance, min_samples) and the pass's
    `samples`.  A NaN compares false: not settled; a count that could leave 2^24 freezes the pixel."""
    tolerance, min_samples = rule
    sums, q = np.asarray(sums, dtype=F), np.asarray(moments, dtype=F)
    n = sums[..., 3]
    with np.errstate(all="ignore"):
        L = luminance(sums[..., :3])
        d = ((n * q).astype(F) - (L * L).astype(F)).astype(F)
        b = (tol2(tolerance) * ((n * n).astype(F) * (n - F(1.0)).astype(F)).astype(F)).astype(F)
        settled = (n >= F(min_samples)) & (d <= b)
        return ~settled & ((n + F(samples)).astype(F) <= LIMIT)


def converge_pass(sums, moments, lin, rule, restart=False):
    """One pass.  `sums` (count, H, W, 4) and `moments` (count, H, W) float32, or None with restart; `lin`
    (count, samples, H, W, 3).  Returns (new sums, new moments, the mask that was marched, the counts after the pass:
    (count,) ints) -- new arrays; an inactive pixel keeps the bit patterns it had."""
    lin = np.asarray(lin, dtype=F)
    count, samples = lin.shape[:2]
    shape = lin.shape[:1] + lin.shape[2:4]
    if restart:
        mask = np.ones(shape, dtype=bool)
        acc = lin[:, 0].astype(F).copy()
        y = luminance(lin[:, 0])
        q = (y * y).astype(F)
        n = np.zeros(shape, dtype=F)
        first = 1
        old_sums, old_moments = np.zeros(shape + (4,), dtype=F), np.zeros(shape, dtype=F)
    else:
        old_sums, old_moments = np.asarray(sums, dtype=F), np.asarray(moments, dtype=F)
        mask = active(old_sums, old_moments, rule, samples)
        acc, q, n = old_sums[..., :3].copy(), old_moments.copy(), old_sums[..., 3].copy()
        first = 0
    with np.errstate(all="ignore"):
        for s in range(first, samples):
            acc = (acc + lin[:, s]).astype(F)
            y = luminance(lin[:, s])
            q = (q + (y * y).astype(F)).astype(F)
        n = (n + F(samples)).astype(F)
    new_sums, new_moments = old_sums.copy(), old_moments.copy()
    new_sums[..., :3][mask] = acc[mask]
    new_sums[..., 3][mask] = n[mask]
    new_moments[mask] = q[mask]
    left = active(new_sums, new_moments, rule, samples)
    return new_sums, new_moments, mask, left.reshape(count, -1).sum(1).astype(np.int64)


def picture(O, sums, encode_mode=1):
    """(count, H, W, 4) uint8: encode(sum / n) of every pixel of a sums plane."""
    with np.errstate(all="ignore"):
        mean = (sums[..., :3] / sums[..., 3:]).astype(F)
    return np.stack([AA.encode(O, m, encode_mode) for m in mean])


def converged(O, passes, rules, encode_mode=1, y0=0, y1=None, sums=None, moments=None, restart=True):
    """Runs `passes` (a list of (count, n, H, W, 3) linear sub-frames) one after another, pass p under rules[p]; the
    first restarts unless planes are given with restart=False.  The counts are those of rows [y0, y1).  Returns a list of
    dicts per pass: sums, moments (rows [y0, y1)), mask (the pixels marched), counts, frames."""
    out = []
    for p, lin in enumerate(passes):
        lin = np.asarray(lin, dtype=F)[:, :, y0:y1]
        if p == 0 and not restart:
            sums, moments = np.asarray(sums, dtype=F), np.asarray(moments, dtype=F)
        sums, moments, mask, counts = converge_pass(sums, moments, lin, rules[p], restart=restart and p == 0)
        out.append(dict(sums=sums, moments=moments, mask=mask, counts=counts, frames=picture(O, sums, encode_mode)))
    return out


def blocks(mask, y0=0):
    """Of one frame's (rows, W) mask: (blocks with no pixel set, blocks partly set, blocks fully set), the 8 x 8 blocks
    of the kernel (block rows start at the band's first row)."""
    rows, w = mask.shape
    none = part = full = 0
    for by in range(0, rows, 8):
        for bx in range(0, w, 8):
            m = mask[by:by + 8, bx:bx + 8]
            if not m.any():
                none += 1
            elif m.all():
                full += 1
            else:
                part += 1
    return none, part, full
