"""The expected frame of k x k supersampling (include/kifs_hip.h, kifs_set_supersampling), from the unmodified oracle:
sample (i, j) of output pixel (x, y) is the oracle's linear colour of pixel (k x + i, k y + j) of the virtual screen
(k W, k H, same aspect_ratio float); the samples are summed in np.float32 in the contract's order (j outer, i inner),
divided by k^2 and encoded with the oracle's own encoder."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from helpers import oracle_uniforms


def virtual_screen(O, screen, k):
    """Screen(k W, k H, aspect) from the product's screen uniform image."""
    return O.Screen(float(k) * screen.width, float(k) * screen.height, screen.aspect_ratio)


def linear_frame(O, screen, camera, options, it, ext=None):
    """(H, W, 3) float32: the oracle's linear colour of every pixel of `screen` (kor_shade_pixel_ext, `ext` an O.Ext for
    the soft-shadow extension or None; ctypes releases the GIL, so the rows run on a few threads)."""
    w, h = int(screen.width), int(screen.height)
    fn = O.lib().kor_shade_pixel_ext
    ext = C.byref(ext) if ext is not None else None
    out = np.zeros((h, w, 3), dtype=np.float32)

    def row(y):
        rgba = (C.c_float * 4)()
        args = (C.byref(screen), C.byref(camera), C.byref(options), C.byref(it), ext)
        for x in range(w):
            fn(*args, x, y, rgba)
            out[y, x] = rgba[:3]

    with ThreadPoolExecutor(16) as ex:
        list(ex.map(row, range(h)))
    return out


def resolve(lin, k):
    """(kH, kW, 3) linear samples -> (H, W, 3) float32 means in the contract's order."""
    kh, kw = lin.shape[:2]
    blocks = lin.reshape(kh // k, k, kw // k, k, 3)  # [y, j, x, i, c]
    acc = blocks[:, 0, :, 0].copy()
    for j in range(k):
        for i in range(k):
            if i or j:
                acc = (acc + blocks[:, j, :, i]).astype(np.float32)
    return (acc / np.float32(k * k)).astype(np.float32)


def encode(O, colour, encode_mode):
    """(H, W, 3) float32 linear -> (H, W, 4) uint8 through kor_encode_channel (alpha 255)."""
    uniq, inv = np.unique(colour.ravel(), return_inverse=True)
    codes = np.array([O.lib().kor_encode_channel(float(v), encode_mode) for v in uniq], dtype=np.uint8)
    rgb = codes[inv].reshape(colour.shape)
    out = np.full(colour.shape[:2] + (4,), 255, dtype=np.uint8)
    out[..., :3] = rgb
    return out


def linear_samples(O, K, screen, camera, gui, iters, k, ext=None):
    """The virtual frame's linear colours for product-side scene objects (ScreenData, CameraData, GuiData or an
    OptionsUniform image)."""
    s, c, o = oracle_uniforms(O, K, (screen, camera, gui))
    return linear_frame(O, virtual_screen(O, s, k), c, o, O.iters(*iters), ext)


def aa_frame(O, K, screen, camera, gui, iters, k, encode_mode=1, lin=None, ext=None):
    if lin is None:
        lin = linear_samples(O, K, screen, camera, gui, iters, k, ext)
    return encode(O, resolve(lin, k), encode_mode)
