"""The expected frame of a jittered accumulated render (include/kifs_hip.h, kifs_render_accumulate_jittered_async), from
the unmodified oracle: sub-frame v of a frame goes through cell (i, j) of the g x g grid inside every pixel, i.e. its
linear colour at output pixel (x, y) is the oracle's (kor_shade_pixel_ext) for pixel (g x + i, g y + j) of the virtual
screen aa_reference.virtual_screen defines -- g W x g H, the same aspect_ratio float -- with that sub-frame's camera and
options; then accumulate_reference.resolve (np.float32 sums in the contract's order, the divide) and aa_reference.encode
(the oracle's own encoder)."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import aa_reference as AA
import accumulate_reference as AR


def _image(u):
    return u.into_buffer_data() if hasattr(u, "into_buffer_data") else u


def linear_view(O, screen, camera, options, it, ext, g, i, j):
    """(H, W, 3) float32: the oracle's linear colour of pixel (g x + i, g y + j) of the virtual screen for every output
    pixel (x, y) of `screen` (oracle structs; `ext` an O.Ext or None)."""
    w, h = int(screen.width), int(screen.height)
    virtual = AA.virtual_screen(O, screen, g)
    fn = O.lib().kor_shade_pixel_ext
    ext = C.byref(ext) if ext is not None else None
    out = np.zeros((h, w, 3), dtype=np.float32)

    def row(y):
        rgba = (C.c_float * 4)()
        args = (C.byref(virtual), C.byref(camera), C.byref(options), C.byref(it), ext)
        for x in range(w):
            fn(*args, g * x + i, g * y + j, rgba)
            out[y, x] = rgba[:3]

    with ThreadPoolExecutor(16) as ex:
        list(ex.map(row, range(h)))
    return out


def cells_of(g, samples, views, cells=None):
    """The cell of every view: `cells` as given, or the supersampling order per frame (cells None: samples == g^2)."""
    if cells is not None:
        assert len(cells) == views
        return [(int(i), int(j)) for i, j in cells]
    assert samples == g * g
    return [((v % samples) % g, (v % samples) // g) for v in range(views)]


def linear_views(O, K, screen, cameras, options, iters, g, cells, samples, ext=None):
    """(views, H, W, 3) float32: the linear frame of every view through its cell.  Arguments as
    accumulate_reference.linear_views, and the grid, the cells (None: supersampling order) and samples per frame."""
    ub = K.uniform_bytes
    s = O.from_bytes(O.Screen, ub(_image(screen)))
    it = O.iters(*iters)
    per_view = isinstance(options, (list, tuple))
    at = cells_of(g, samples, len(cameras), cells)
    out = []
    for v in range(len(cameras)):
        c = O.from_bytes(O.Camera, ub(_image(cameras[v])))
        o = O.from_bytes(O.Options, ub(_image(options[v] if per_view else options)))
        out.append(linear_view(O, s, c, o, it, ext, g, *at[v]))
    return np.stack(out)


def jittered_frames(O, K, screen, cameras, options, iters, samples, g, cells=None, encode_mode=1, lin=None, ext=None, y0=0,
                    y1=None):
    """(count, rows, W, 4) uint8: the frames kifs_render_accumulate_jittered_async must write for these sub-frames."""
    if lin is None:
        lin = linear_views(O, K, screen, cameras, options, iters, g, cells, samples, ext)
    mean = AR.resolve(lin, samples)[:, y0:y1]
    return np.stack([AA.encode(O, m, encode_mode) for m in mean])
