"""The expected frame of an accumulated render (include/kifs_hip.h, kifs_render_accumulate_async), from the unmodified
oracle: sub-frame s of a frame is the oracle's linear colour of every pixel for that sub-frame's camera and options
(aa_reference.linear_frame on the plain screen: k = 1); the sub-frames are summed in np.float32 in the contract's order
(acc = c_0, then + c_1, + c_2, ..), divided by np.float32(samples) and encoded with the oracle's own encoder."""
import numpy as np

import aa_reference as AA


def _image(u):
    return u.into_buffer_data() if hasattr(u, "into_buffer_data") else u


def linear_views(O, K, screen, cameras, options, iters, ext=None):
    """(views, H, W, 3) float32: the linear frame of every view.  `cameras`: CameraData objects or CameraUniform images;
    `options`: one GuiData / options image for all views, or a list of them, one per view."""
    ub = K.uniform_bytes
    s = O.from_bytes(O.Screen, ub(_image(screen)))
    it = O.iters(*iters)
    per_view = isinstance(options, (list, tuple))
    out = []
    for v in range(len(cameras)):
        c = O.from_bytes(O.Camera, ub(_image(cameras[v])))
        o = O.from_bytes(O.Options, ub(_image(options[v] if per_view else options)))
        out.append(AA.linear_frame(O, s, c, o, it, ext))
    return np.stack(out)


def resolve(lin, samples):
    """(count * samples, H, W, 3) linear sub-frames -> (count, H, W, 3) float32 means in the contract's order."""
    views = lin.shape[0]
    assert views % samples == 0
    groups = lin.reshape(views // samples, samples, *lin.shape[1:])
    acc = groups[:, 0].astype(np.float32).copy()
    for s in range(1, samples):
        acc = (acc + groups[:, s]).astype(np.float32)
    return (acc / np.float32(samples)).astype(np.float32)


def accumulate_frames(O, K, screen, cameras, options, iters, samples, encode_mode=1, lin=None, ext=None, y0=0, y1=None):
    """(count, rows, W, 4) uint8: the frames kifs_render_accumulate_async must write for these sub-frames."""
    if lin is None:
        lin = linear_views(O, K, screen, cameras, options, iters, ext)
    mean = resolve(lin, samples)[:, y0:y1]
    return np.stack([AA.encode(O, m, encode_mode) for m in mean])
