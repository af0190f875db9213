"""The expected frame of adaptive anti-aliasing (include/kifs_hip.h, kifs_render_adaptive_async) from the unmodified
oracle and the geometry contract's CPU restatement: the edge mask E from the geometry plane in NumPy float32, in the
contract's operation order; the plain oracle frame where E is false; where it is true, the k^2 samples of the virtual
screen (kor_shade_pixel) summed as aa_reference.resolve sums them and encoded with the oracle's encoder."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import aa_reference as AA
import geometry_reference as GR
from helpers import oracle_uniforms

MISS_T = 0x7f800000
SILHOUETTE = (-2.0, float("inf"))  # thresholds no two hits can fail: only hit against miss is an edge
DEFAULT = (0.9, 0.05)
ALL_HITS = (2.0, 0.0)              # no two hits can pass: every hit with a neighbour is an edge


def _pair(p, q, normal_cos, depth_rel):
    """pair(p, q) of the contract for two (..., 4) float32 texel arrays of one shape."""
    nc, dr = np.float32(normal_cos), np.float32(depth_rel)
    tp, tq = p[..., 3], q[..., 3]
    hp, hq = tp.view(np.uint32) != MISS_T, tq.view(np.uint32) != MISS_T
    with np.errstate(all="ignore"):
        d = ((p[..., 0] * q[..., 0]).astype(np.float32) + (p[..., 1] * q[..., 1]).astype(np.float32)).astype(np.float32)
        d = (d + (p[..., 2] * q[..., 2]).astype(np.float32)).astype(np.float32)
        apart = np.abs((tp - tq).astype(np.float32)) > (dr * np.fmin(tp, tq)).astype(np.float32)
        both = ~(d >= nc) | apart
    return (hp != hq) | (hp & hq & both)


def edge_mask(geom, normal_cos, depth_rel):
    """E(p) for a (H, W, 4) float32 geometry plane: the OR of pair(p, q) over p's 4-neighbours inside the frame."""
    g = np.ascontiguousarray(geom, dtype=np.float32)
    e = np.zeros(g.shape[:2], dtype=bool)
    e[:, 1:] |= _pair(g[:, 1:], g[:, :-1], normal_cos, depth_rel)   # q = (x - 1, y)
    e[:, :-1] |= _pair(g[:, :-1], g[:, 1:], normal_cos, depth_rel)  # q = (x + 1, y)
    e[1:] |= _pair(g[1:], g[:-1], normal_cos, depth_rel)            # q = (x, y - 1)
    e[:-1] |= _pair(g[:-1], g[1:], normal_cos, depth_rel)           # q = (x, y + 1)
    return e


def resolved_pixels(O, K, screen, camera, gui, iters, k, pixels, ext=None):
    """(N, 3) float32: the contract's mean of the k^2 linear samples of each (y, x) of `pixels` (N, 2); `ext`: an O.Ext
    for the soft-shadow extension or None."""
    s, c, o = oracle_uniforms(O, K, (screen, camera, gui))
    virt, it = AA.virtual_screen(O, s, k), O.iters(*iters)
    fn = O.lib().kor_shade_pixel_ext
    e = C.byref(ext) if ext is not None else None
    out = np.zeros((len(pixels), 3), dtype=np.float32)

    def one(n):
        y, x = int(pixels[n][0]), int(pixels[n][1])
        rgba = (C.c_float * 4)()
        acc = None
        for j in range(k):
            for i in range(k):
                fn(C.byref(virt), C.byref(c), C.byref(o), C.byref(it), e, k * x + i, k * y + j, rgba)
                v = np.array(rgba[:3], dtype=np.float32)
                acc = v if acc is None else (acc + v).astype(np.float32)  # as aa_reference.resolve: s = 0 first
        out[n] = (acc / np.float32(k * k)).astype(np.float32)

    with ThreadPoolExecutor(16) as ex:
        list(ex.map(one, range(len(pixels))))
    return out


def geometry(O, K, screen, camera, gui, iters):
    return GR.geometry_frame(O, K, screen, camera, gui, iters)[0]


def expected_frame(O, K, screen, camera, gui, iters, k, normal_cos, depth_rel, encode=1, geom=None, means=None, ext=None):
    """(frame (H, W, 4) uint8, mask (H, W) bool).  `geom`: the scene's geometry plane when the caller has it; `means`:
    a dict the resolved means of this (scene, k, mask) are kept in across encodes; `ext`: an O.Ext -- the soft-shadow
    extension changes the colours on and off the mask, never the mask (the geometry is the primary ray's)."""
    s, c, o = oracle_uniforms(O, K, (screen, camera, gui))
    frame = O.render(s, c, o, O.iters(*iters), encode=encode, ext=ext).copy()
    if geom is None:
        geom = geometry(O, K, screen, camera, gui, iters)
    mask = edge_mask(geom, normal_cos, depth_rel)
    pixels = np.argwhere(mask)
    if len(pixels):
        key = (k, mask.tobytes())
        if means is None or key not in means:
            lin = resolved_pixels(O, K, screen, camera, gui, iters, k, pixels, ext)
            if means is not None:
                means[key] = lin
        else:
            lin = means[key]
        frame[mask] = AA.encode(O, lin.reshape(-1, 1, 3), encode).reshape(-1, 4)
    return frame, mask
