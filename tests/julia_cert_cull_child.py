"""Child process of tests/test_gpu_julia_cert_cull.py: renders every launch of tests/julia_cert_cull_cases.py in one kernel
form, with the certified cull on or off.  The KIFS_TUNING knobs that decide both come with the environment and are read
once per process, hence one process per combination.  Writes, per launch, the debug tuple, the first frame of every
distinct view and whether every other copy of a view equals it; with EXTRAS, the other entry points' frames as well.

    python tests/julia_cert_cull_child.py OUT.npz [extras]
"""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent), str(HERE)]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import julia_cert_cull_cases as X  # noqa: E402
import kifs_raymarching_amd as K  # noqa: E402

SENT = 0x5A  # a pixel no kernel wrote keeps alpha 0x5a, which no encode produces


def _scene(gs, scene):
    w, h = X.SCENES[scene][3]
    gs.update_screen_data(K.ScreenData(w, h))
    gs.update_options(X.options(K, scene))
    gs.set_iters(*X.iters(scene))
    gs.set_extensions(soft_shadow=False)
    gs.set_supersampling(1)
    return w, h


def batches(gs, result):
    stream = torch.cuda.Stream()
    for i, (scene, views) in enumerate(X.launches()):
        w, h = _scene(gs, scene)
        cams = [X.view(K, v).u for v in views]
        n = len(cams)
        outs = torch.full((n, h, w, 4), SENT, dtype=torch.uint8, device="cuda:0")
        gs.render_batch_async([outs[v] for v in range(n)], cams, stream=stream)
        stream.synchronize()
        kernel = (gs.debug_last_kernel(), gs.debug_last_group_tiles(), gs.debug_last_round_steps())
        first = {}
        for k, v in enumerate(views):
            first.setdefault(v, k)
        same = all(bool((outs[k] == outs[first[v]]).all()) for k, v in enumerate(views))
        result[f"L{i}_kernel"] = np.array([kernel[0]])
        result[f"L{i}_shape"] = np.array(kernel[1:], dtype=np.int32)
        result[f"L{i}_views"] = np.array(sorted(first), dtype=np.int32)
        result[f"L{i}_frames"] = np.stack([outs[first[v]].cpu().numpy() for v in sorted(first)])
        result[f"L{i}_copies_equal"] = np.array([same])
        print(f"{scene} x{n}: {kernel}", flush=True)


def extras(gs, result):
    scene = X.EXTRA_SCENE
    w, h = _scene(gs, scene)
    cam5, cam2 = X.view(K, 0).u, X.view(K, 1).u
    # a batch of 3 poses in one launch, whatever form the rules give it
    outs = torch.full((3, h, w, 4), SENT, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.Stream()
    gs.render_batch_async([outs[v] for v in range(3)], [X.view(K, v).u for v in (0, 1, 2)], stream=stream)
    stream.synchronize()
    result["batch3"] = outs.cpu().numpy()
    # a band
    gs.set_raw_uniforms(camera=cam2)
    result["band"] = np.asarray(gs.render(y0=X.BAND[0], y1=X.BAND[1]))
    # supersampling k = 2
    gs.set_raw_uniforms(camera=cam5)
    gs.set_supersampling(2)
    result["ssaa2"] = np.asarray(gs.render())
    gs.set_supersampling(1)
    # the geometry output, both far views in one launch
    colour, geom = gs.render_geometry_batch([cam5, cam2])
    torch.cuda.synchronize()
    result["geometry_colour"] = colour.cpu().numpy()
    result["geometry"] = geom.cpu().numpy()
    # adaptive anti-aliasing
    colour, counts = gs.render_adaptive_batch([cam5, cam2], k=2)
    torch.cuda.synchronize()
    result["adaptive"] = colour.cpu().numpy()
    result["adaptive_counts"] = counts.cpu().numpy()
    # animated launches: frames with their own constants
    for a, constants in enumerate(X.ANIMATIONS):
        opts = [X.options(K, scene, c) for c in constants]
        frames = gs.render_animation(opts, cameras=[cam5, cam2])
        torch.cuda.synchronize()
        result[f"animation{a}"] = frames.cpu().numpy()
    # an accumulated launch of 4 sub-frames, and one whose sub-frames bring their own constants
    sub = [K.CameraData(origin_distance=d, min_distance=0.05, phi=p, theta=t) for d, p, t in X.ACCUMULATE_VIEWS]
    frames = gs.render_accumulate(sub, 4)
    torch.cuda.synchronize()
    result["accumulate"] = frames.cpu().numpy()
    opts = [X.options(K, scene, c) for c in (X.HEADLINE_C, X.SMALL_C, X.HEADLINE_C, X.REFERENCE_C)]
    frames = gs.render_accumulate(sub, 4, options=opts)
    torch.cuda.synchronize()
    result["accumulate_options"] = frames.cpu().numpy()


def main(out_path, with_extras):
    result = {}
    with K.GraphicState(0) as gs:
        batches(gs, result)
        if with_extras:
            extras(gs, result)
    np.savez(out_path, **result)


if __name__ == "__main__":
    main(sys.argv[1], len(sys.argv) > 2 and sys.argv[2] == "extras")
